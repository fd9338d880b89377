// Stand-alone driver of the host-side checks of PillarVFE and the BEV scatter (include/modest_hip.h, "a38"): every argument
// refusal of modest_pillar_vfe / modest_pillar_vfe_backward / modest_pillar_scatter / modest_pillar_scatter_backward /
// modest_pillar_vfe_workspace_bytes, and the calls that have nothing to do.  A refused call launches nothing, so the program needs
// no GPU; it is meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Imodest_amd/csrc tools/pillar_vfe_host_check.cpp modest_amd/csrc/pillar_vfe.hip \
//         -o pillar_vfe_host_check && ./pillar_vfe_host_check
//
// pillar_vfe.hip needs nothing of the library but its error text, which csrc/ctx.hip keeps together with the context; the two
// functions are restated below so that the translation unit under test links on its own.  It prints one line per check and
// exits 0 when every check holds.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "modest_hip.h"

static char g_err[512];

void modest_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *modest_last_error(void) { return g_err; }

static int failures = 0;

static void expect(bool ok, const char *what) {
    std::printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++failures;
}

static bool refused(int64_t rc, const char *needle) { return rc != 0 && std::strstr(modest_last_error(), needle) != nullptr; }

int main() {
    expect(modest_pillar_vfe_run() == 32 && modest_pillar_vfe_group() == 64, "a run of 32 pillars, a group of 64 runs");
    // host memory stands in for device memory: a refused call never touches it
    alignas(256) static float buf[256];
    void *p = buf;
    void *odd2 = reinterpret_cast<char *>(buf) + 2, *odd4 = reinterpret_cast<char *>(buf) + 4;
    const float geometry[6] = {0.25f, 0.25f, 8.f, -0.625f, -0.5f, 1.f};
    const int64_t big = ((int64_t)1 << 20);

    struct Fwd {
        int64_t P = 4; int S = 3, Cp = 4, C = 8, parts = 7, ncode = 0, ccode = 0, training = 1;
        void *voxels, *num, *coords, *W, *rm, *rv, *tracked, *out, *winner, *sums, *stat, *ws;
        const float *geo; double eps = 1e-3; int64_t bytes;
    };
    auto fresh = [&]() { Fwd a; a.voxels = a.num = a.coords = a.W = a.rm = a.rv = a.tracked = a.out = a.winner = a.sums = a.stat = a.ws = p;
                         a.geo = geometry; a.bytes = big; return a; };
    auto fwd = [&](const Fwd &a) {
        return modest_pillar_vfe(a.P, a.S, a.Cp, a.C, a.parts, (const float *)a.voxels, a.num, a.ncode, a.coords, a.ccode, a.geo,
                                 (const float *)a.W, (const float *)a.W, (const float *)a.W, (float *)a.rm, (float *)a.rv,
                                 (int64_t *)a.tracked, a.eps, 0.01, a.training, (float *)a.out, (uint8_t *)a.winner, (double *)a.sums,
                                 (float *)a.stat, a.ws, a.bytes, nullptr);
    };
    Fwd a = fresh(); a.P = -1;               expect(refused(fwd(a), "n_pillars >= 0"), "vfe: n_pillars = -1");
    a = fresh(); a.S = 0;                    expect(refused(fwd(a), "slots of a pillar between 1 and 255"), "vfe: slots = 0");
    a = fresh(); a.S = 256;                  expect(refused(fwd(a), "slots of a pillar between 1 and 255"), "vfe: slots = 256");
    a = fresh(); a.C = 0;                    expect(refused(fwd(a), "output channels between 1 and 64"), "vfe: channels = 0");
    a = fresh(); a.C = 65;                   expect(refused(fwd(a), "output channels between 1 and 64"), "vfe: channels = 65");
    a = fresh(); a.parts = 16;               expect(refused(fwd(a), "parts is a mask"), "vfe: parts = 16");
    a = fresh(); a.parts = -1;               expect(refused(fwd(a), "parts is a mask"), "vfe: parts = -1");
    a = fresh(); a.Cp = 2;                   expect(refused(fwd(a), "point features between 3 and 19"), "vfe: 2 point features");
    a = fresh(); a.Cp = 20; a.parts = 0;     expect(refused(fwd(a), "point features between 3 and 19"), "vfe: 20 point features");
    a = fresh(); a.Cp = 3; a.parts = 0;      expect(refused(fwd(a), "features of a point between 1 and 16"), "vfe: K = 0");
    a = fresh(); a.Cp = 10; a.parts = 15;    expect(refused(fwd(a), "features of a point between 1 and 16"), "vfe: K = 17");
    a = fresh(); a.P = ((int64_t)1 << 31) / 3 + 1; expect(refused(fwd(a), "at most 2^31 - 1 rows"), "vfe: n_pillars * slots = 2^31 + 2");
    a = fresh(); a.P = INT64_MAX; a.S = 255; expect(refused(fwd(a), "at most 2^31 - 1 rows"), "vfe: INT64_MAX pillars");
    a = fresh(); a.ncode = 3;                expect(refused(fwd(a), "dtype code"), "vfe: num dtype code 3");
    a = fresh(); a.ccode = -1;               expect(refused(fwd(a), "dtype code"), "vfe: coords dtype code -1");
    a = fresh(); a.geo = nullptr;            expect(refused(fwd(a), "NULL geometry"), "vfe: no geometry");
    a = fresh(); a.eps = -1.0;               expect(refused(fwd(a), "eps >= 0"), "vfe: eps = -1");
    a = fresh(); a.P = 1; a.S = 1;           expect(refused(fwd(a), "more than one row"), "vfe: one row in training mode");
    a = fresh(); a.training = 0; a.rm = a.rv = nullptr; expect(refused(fwd(a), "running_mean and running_var in eval mode"), "vfe: eval without running buffers");
    a = fresh(); a.rv = nullptr;             expect(refused(fwd(a), "come together"), "vfe: running_mean without running_var");
    a = fresh(); a.voxels = nullptr;         expect(refused(fwd(a), "NULL buffer"), "vfe: no voxels");
    a = fresh(); a.out = nullptr;            expect(refused(fwd(a), "NULL buffer"), "vfe: no output");
    a = fresh(); a.winner = nullptr;         expect(refused(fwd(a), "NULL buffer (winner"), "vfe: no winner in training mode");
    a = fresh(); a.ws = nullptr;             expect(refused(fwd(a), "NULL buffer (winner"), "vfe: no workspace in training mode");
    a = fresh(); a.voxels = odd2;            expect(refused(fwd(a), "unaligned buffer"), "vfe: unaligned voxels");
    a = fresh(); a.ncode = 2; a.num = odd4;  expect(refused(fwd(a), "unaligned buffer"), "vfe: int64 counts on a 4-byte boundary");
    a = fresh(); a.sums = odd4;              expect(refused(fwd(a), "unaligned buffer"), "vfe: float64 sums on a 4-byte boundary");
    a = fresh(); a.bytes = 8;                expect(refused(fwd(a), "workspace of modest_pillar_vfe_workspace_bytes"), "vfe: a workspace of 8 bytes");
    a = fresh(); a.P = 0; a.training = 0; a.voxels = a.out = nullptr; expect(fwd(a) == 0, "vfe: nothing to do in eval mode is fine");

    auto bwd = [&](int64_t P, int S, int C, int parts, const void *voxels, const void *grad, void *dW, void *ws, int64_t bytes) {
        return modest_pillar_vfe_backward(P, S, 4, C, parts, (const float *)voxels, p, 0, p, 0, geometry, (const float *)p,
                                          (const float *)p, (const float *)p, (const uint8_t *)p, (const float *)grad,
                                          (const double *)p, (const float *)p, (float *)dW, (float *)p, (float *)p, ws, bytes, nullptr);
    };
    expect(refused(bwd(4, 3, 0, 7, p, p, p, p, big), "output channels between 1 and 64"), "backward: channels = 0");
    expect(refused(bwd(4, 256, 8, 7, p, p, p, p, big), "slots of a pillar"), "backward: slots = 256");
    expect(refused(bwd(4, 3, 8, 31, p, p, p, p, big), "parts is a mask"), "backward: parts = 31");
    expect(refused(bwd(1, 1, 8, 7, p, p, p, p, big), "more than one row"), "backward: one row");
    expect(refused(bwd(0, 3, 8, 7, p, p, p, p, big), "more than one row"), "backward: no pillar");
    expect(refused(bwd(4, 3, 8, 7, nullptr, p, p, p, big), "NULL buffer"), "backward: no voxels");
    expect(refused(bwd(4, 3, 8, 7, p, nullptr, p, p, big), "NULL buffer"), "backward: no grad_out");
    expect(refused(bwd(4, 3, 8, 7, p, p, nullptr, p, big), "NULL buffer"), "backward: no grad_weight");
    expect(refused(bwd(4, 3, 8, 7, p, p, p, nullptr, big), "NULL buffer"), "backward: no workspace");
    expect(refused(bwd(4, 3, 8, 7, p, odd2, p, p, big), "unaligned buffer"), "backward: unaligned grad_out");
    expect(refused(bwd(4, 3, 8, 7, p, p, p, odd4, big), "unaligned buffer"), "backward: a workspace on a 4-byte boundary");
    expect(refused(bwd(4, 3, 8, 7, p, p, p, p, 8), "workspace of modest_pillar_vfe_workspace_bytes"), "backward: a workspace of 8 bytes");

    expect(refused(modest_pillar_vfe_workspace_bytes(-1, 8, 10), "n_pillars between"), "workspace: n_pillars = -1");
    expect(refused(modest_pillar_vfe_workspace_bytes(4, 65, 10), "output channels"), "workspace: channels = 65");
    expect(refused(modest_pillar_vfe_workspace_bytes(4, 8, 17), "features of a point"), "workspace: K = 17");
    expect(modest_pillar_vfe_workspace_bytes(33, 8, 10) == 8 * (2 * 8 + 10 * 8 + 10) * 3, "workspace: two runs and a group of 33 pillars");

    auto sc = [&](int64_t P, int C, int B, int ny, int nx, const void *feat, const void *coords, int code, void *canvas) {
        return modest_pillar_scatter(P, C, B, ny, nx, (const float *)feat, coords, code, (float *)canvas, nullptr);
    };
    expect(refused(sc(-1, 8, 1, 2, 2, p, p, 0, p), "n_pillars between"), "scatter: n_pillars = -1");
    expect(refused(sc(4, 0, 1, 2, 2, p, p, 0, p), "channels between 1 and 64"), "scatter: channels = 0");
    expect(refused(sc(4, 65, 1, 2, 2, p, p, 0, p), "channels between 1 and 64"), "scatter: channels = 65");
    expect(refused(sc(4, 8, -1, 2, 2, p, p, 0, p), "batch between 0 and 65535"), "scatter: batch = -1");
    expect(refused(sc(4, 8, 65536, 2, 2, p, p, 0, p), "batch between 0 and 65535"), "scatter: batch = 65536");
    expect(refused(sc(4, 8, 1, 0, 2, p, p, 0, p), "a grid of ny, nx >= 1"), "scatter: ny = 0");
    expect(refused(sc(4, 8, 1, 65536, 65536, p, p, 0, p), "a grid of ny, nx >= 1"), "scatter: 2^32 cells");
    expect(refused(sc(4, 8, 1, 2, 2, p, p, 3, p), "dtype code"), "scatter: coords dtype code 3");
    expect(refused(sc(4, 8, 1, 2, 2, nullptr, p, 0, p), "NULL buffer"), "scatter: no features");
    expect(refused(sc(4, 8, 1, 2, 2, p, nullptr, 0, p), "NULL buffer"), "scatter: no coords");
    expect(refused(sc(4, 8, 1, 2, 2, p, p, 0, nullptr), "NULL buffer"), "scatter: no canvas");
    expect(refused(sc(4, 8, 1, 2, 2, p, odd4, 2, p), "unaligned buffer"), "scatter: int64 coords on a 4-byte boundary");
    expect(refused(sc(4, 8, 1, 2, 2, p, p, 0, odd2), "unaligned buffer"), "scatter: unaligned canvas");
    expect(sc(0, 8, 0, 2, 2, nullptr, nullptr, 0, nullptr) == 0 && sc(4, 8, 0, 2, 2, p, p, 0, nullptr) == 0, "scatter: no sample is fine");

    auto sb = [&](int64_t P, int C, int B, const void *grad_canvas, const void *coords, int code, void *grad) {
        return modest_pillar_scatter_backward(P, C, B, 2, 2, (const float *)grad_canvas, coords, code, (float *)grad, nullptr);
    };
    expect(refused(sb(4, 65, 1, p, p, 0, p), "channels between 1 and 64"), "scatter backward: channels = 65");
    expect(refused(sb(4, 8, 65536, p, p, 0, p), "batch between 0 and 65535"), "scatter backward: batch = 65536");
    expect(refused(sb(4, 8, 1, nullptr, p, 0, p), "NULL buffer"), "scatter backward: no grad_canvas");
    expect(refused(sb(4, 8, 1, p, p, 0, nullptr), "NULL buffer"), "scatter backward: no grad_features");
    expect(refused(sb(4, 8, 1, p, odd4, 2, p), "unaligned buffer"), "scatter backward: int64 coords on a 4-byte boundary");
    expect(sb(0, 8, 1, p, nullptr, 0, nullptr) == 0, "scatter backward: no pillar is fine");
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
