// Stand-alone driver of the host-side checks of the optimiser step (include/modest_hip.h, "a40"): every refusal of
// modest_optim_step / modest_optim_norm_step / modest_optim_clip / modest_optim_grad_norm / modest_optim_workspace_bytes on the
// two host tables.  A refused call launches nothing and never reaches the staging ring, so the program needs no GPU; it is meant
// to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Imodest_amd/csrc tools/optim_step_host_check.cpp modest_amd/csrc/optim_step.hip \
//         -o optim_step_host_check && ./optim_step_host_check
//
// optim_step.hip needs the library's error text and the context's staging ring (csrc/ctx.hip); they are restated below so that
// the translation unit under test links on its own -- the ring as two functions that fail, which no check here may reach.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "common.h"

static char g_err[512];
static int ring_calls = 0;

void modest_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char *modest_last_error(void) { return g_err; }
int modest_ctx_stage_slot(modest_ctx *, size_t, void **) { ++ring_calls; return MODEST_ERR_HIP; }
int modest_ctx_stage_commit(modest_ctx *, hipStream_t) { ++ring_calls; return MODEST_ERR_HIP; }

struct Static { uint64_t p, m, v; int64_t n; int32_t first_chunk, pad; };
struct Step { uint64_t g; float s[8]; uint32_t flags; int32_t norm_first; };
static_assert(sizeof(Static) == 40 && sizeof(Step) == 48, "the table layout of include/modest_hip.h");

static int failures = 0;
static void expect(bool ok, const char *what) {
    std::printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++failures;
}
static bool refused(int64_t rc, const char *needle) { return rc != 0 && std::strstr(modest_last_error(), needle) != nullptr; }

int main() {
    const int CH = modest_optim_chunk();
    expect(CH == 4096, "a chunk of 4096 elements");
    alignas(256) static float buf[4096];          // host memory stands in for device memory: a refused call never touches it
    modest_ctx *ctx = reinterpret_cast<modest_ctx *>(buf);
    const uint64_t a = reinterpret_cast<uint64_t>(buf);
    const int64_t big = 1 << 20;
    float *norm = buf;

    auto table = [&](Static st[3], Step sp[3]) {   // 3 tensors of 5, 4097 and 7 elements: 1 + 2 + 1 chunks; the last without a gradient
        const int64_t n[3] = {5, CH + 1, 7};
        int32_t chunk = 0, part = 0;
        for (int t = 0; t < 3; ++t) {
            const int32_t own = (int32_t)((n[t] + CH - 1) / CH);
            st[t] = Static{a, a + 64, a + 128, n[t], chunk, 0};
            sp[t] = Step{t < 2 ? a + 192 : 0, {1, 0.1f, 0.9f, 0.99f, 0.01f, 1, 1e-8f, -1e-3f}, 0, t < 2 ? part : -1};
            chunk += own;
            part += t < 2 ? own : 0;
        }
    };
    auto step = [&](int64_t T, int64_t chunks, const Static *st, const Step *sp, void *ws, int64_t bytes) {
        return modest_optim_step(ctx, T, chunks, st, sp, 1, ws, bytes, nullptr);
    };
    Static st[3];
    Step sp[3];
    table(st, sp);
    expect(refused(modest_optim_step(nullptr, 3, 4, st, sp, 1, buf, big, nullptr), "no context"), "step: no context");
    expect(refused(step(0, 0, st, sp, buf, big), "1 <= tensors"), "step: no tensor");
    expect(refused(step((1 << 20) + 1, (1 << 20) + 1, st, sp, buf, big), "1 <= tensors"), "step: 2^20 + 1 tensors");
    expect(refused(step(3, 2, st, sp, buf, big), "1 <= tensors"), "step: fewer chunks than tensors");
    expect(refused(step(3, (int64_t)1 << 31, st, sp, buf, big), "1 <= tensors"), "step: 2^31 chunks");
    expect(refused(step(3, 4, nullptr, sp, buf, big), "two host tables"), "step: no static table");
    expect(refused(step(3, 4, st, nullptr, buf, big), "two host tables"), "step: no step table");
    expect(refused(step(3, 4, st, sp, nullptr, big), "256-byte aligned workspace"), "step: no workspace");
    expect(refused(step(3, 4, st, sp, buf + 1, big), "256-byte aligned workspace"), "step: a workspace on a 4-byte boundary");
    expect(refused(step(3, 4, st, sp, buf, 64), "workspace smaller"), "step: a workspace of 64 bytes");
    expect(refused(step(3, 5, st, sp, buf, big), "n_chunks is not the sum"), "step: one chunk too many");
    expect(refused(step(3, 3, st, sp, buf, big), "more chunks than n_chunks"), "step: one chunk too few");
    table(st, sp); st[1].n = 0;             expect(refused(step(3, 4, st, sp, buf, big), "without elements"), "step: a tensor of 0 elements");
    table(st, sp); st[1].n = -3;            expect(refused(step(3, 4, st, sp, buf, big), "without elements"), "step: a tensor of -3 elements");
    table(st, sp); st[2].first_chunk = 2;   expect(refused(step(3, 4, st, sp, buf, big), "first_chunk is not the running sum"), "step: a first chunk that is too small");
    table(st, sp); st[1].n = 2 * CH + 1;    expect(refused(step(3, 4, st, sp, buf, big), "first_chunk is not the running sum"), "step: a tensor longer than its chunks");
    table(st, sp); st[0].p = 0;             expect(refused(step(3, 4, st, sp, buf, big), "parameter pointer"), "step: no parameter");
    table(st, sp); st[0].p = a + 2;         expect(refused(step(3, 4, st, sp, buf, big), "parameter pointer"), "step: a parameter on a 2-byte boundary");
    table(st, sp); st[1].m = 0;             expect(refused(step(3, 4, st, sp, buf, big), "state pointer"), "step: a gradient without exp_avg");
    table(st, sp); st[1].v = a + 1;         expect(refused(step(3, 4, st, sp, buf, big), "state pointer"), "step: exp_avg_sq on an odd address");
    table(st, sp); sp[0].g = a + 3;         expect(refused(step(3, 4, st, sp, buf, big), "gradient that is not 4-byte aligned"), "step: a gradient on an odd address");
    table(st, sp); sp[1].norm_first = 0;    expect(refused(step(3, 4, st, sp, buf, big), "norm_first is not the running sum"), "step: two tensors on one partial");
    table(st, sp); sp[2].norm_first = 3;    expect(refused(step(3, 4, st, sp, buf, big), "must be -1"), "step: a partial for a tensor without a gradient");
    table(st, sp); st[2].m = st[2].v = 0;   expect(step(3, 4, st, sp, buf, big) == MODEST_ERR_HIP && ring_calls == 1, "step: a valid table reaches the ring (no state needed without a gradient)");
    table(st, sp);
    expect(refused(modest_optim_norm_step(ctx, 3, 4, st, sp, 1, 10.f, 0, nullptr, buf, big, nullptr), "no output"), "norm_step: no output");
    expect(refused(modest_optim_clip(ctx, 3, 4, st, sp, 1, 10.f, 0, nullptr, buf, big, nullptr), "no output"), "clip: no output");
    expect(refused(modest_optim_grad_norm(ctx, 3, 4, st, sp, 1, nullptr, buf, big, nullptr), "no output"), "grad_norm: no output");
    expect(refused(modest_optim_clip(ctx, 3, 3, st, sp, 1, 10.f, 0, norm, buf, big, nullptr), "more chunks than n_chunks"), "clip: one chunk too few");
    st[0].p = st[0].m = st[0].v = 0;        // the norm and the clip read no state
    ring_calls = 0;
    expect(modest_optim_clip(ctx, 3, 4, st, sp, 1, 10.f, 0, norm, buf, big, nullptr) == MODEST_ERR_HIP && ring_calls == 1, "clip: a valid table without state reaches the ring");
    expect(refused(modest_optim_norm_step(ctx, 3, 4, st, sp, 1, 10.f, 0, norm, buf, big, nullptr), "parameter pointer"), "norm_step: the same table is refused");
    expect(refused(modest_optim_workspace_bytes(0, 0), "1 <= tensors"), "workspace: no tensor");
    expect(refused(modest_optim_workspace_bytes(3, 2), "1 <= tensors"), "workspace: fewer chunks than tensors");
    expect(modest_optim_workspace_bytes(3, 4) == 256 + 256 + 256 + 256, "workspace: three tensors, four chunks");
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
