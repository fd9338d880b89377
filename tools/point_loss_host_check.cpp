// Stand-alone driver of the host-side checks of the point-head loss (include/modest_hip.h, "a36"): the workspace arithmetic of
// modest_point_loss_workspace_bytes and every argument refusal of modest_point_loss / modest_point_loss_backward.  A refused
// call launches nothing, so the program needs no GPU; it is meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Imodest_amd/csrc tools/point_loss_host_check.cpp modest_amd/csrc/point_loss.hip \
//         -o point_loss_host_check && ./point_loss_host_check
//
// point_loss.hip needs nothing of the library but its error text, which csrc/ctx.hip keeps together with the context; the two
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

static bool refused(int rc, const char *needle) { return rc != 0 && std::strstr(modest_last_error(), needle) != nullptr; }

int main() {
    const int64_t max_rows = modest_point_loss_max_rows();
    expect(max_rows == (int64_t)1 << 24, "max_rows is 2^24");
    // the counter's 256 bytes, then three float partials per workgroup of 256 points, rounded up to 256 bytes
    expect(modest_point_loss_workspace_bytes(0) == 512, "workspace(0) = 256 + 256");
    expect(modest_point_loss_workspace_bytes(1) == 512, "workspace(1) = 256 + 256");
    expect(modest_point_loss_workspace_bytes(256 * 21) == 512, "workspace(21 workgroups) = 256 + 256");
    expect(modest_point_loss_workspace_bytes(256 * 21 + 1) == 768, "workspace(22 workgroups) = 256 + 512");
    expect(modest_point_loss_workspace_bytes(max_rows) == 256 + 12 * 65536, "workspace(2^24)");
    expect(modest_point_loss_workspace_bytes(max_rows + 1) < 0, "workspace(2^24 + 1) is refused");
    expect(modest_point_loss_workspace_bytes(-1) < 0, "workspace(-1) is refused");
    expect(modest_point_loss_workspace_bytes(INT64_MAX) < 0 && modest_point_loss_workspace_bytes(INT64_MIN) < 0,
           "workspace(INT64_MAX / INT64_MIN) is refused");

    // host memory stands in for device memory: a refused call never touches it
    alignas(256) static float buf[256];
    float *p = buf;
    void *ws = buf;
    auto call = [&](int64_t n, int c, int code, const float *part, const float *part_t, const float *box, const float *box_t,
                    const float *cw, float *gc, float *gp, float *gb, float *table, void *w, int64_t wbytes) {
        return modest_point_loss(n, c, code, p, p, 0, part, part_t, box, box_t, cw, 0.1f, 1.f, 1.f, 1.f, gc, gp, gb, table, w, wbytes, nullptr);
    };
    expect(refused(call(-1, 1, 8, 0, 0, p, p, p, 0, 0, 0, p, ws, 1024), "n_rows between 0 and 2^24"), "n_rows = -1");
    expect(refused(call(max_rows + 1, 1, 8, 0, 0, p, p, p, 0, 0, 0, p, ws, 1024), "n_rows between 0 and 2^24"), "n_rows = 2^24 + 1");
    expect(refused(call(4, 0, 8, 0, 0, p, p, p, 0, 0, 0, p, ws, 1024), "num_class between 1 and 32"), "num_class = 0");
    expect(refused(call(4, 33, 8, 0, 0, p, p, p, 0, 0, 0, p, ws, 1024), "num_class between 1 and 32"), "num_class = 33");
    expect(refused(call(4, 1, 0, 0, 0, p, p, p, 0, 0, 0, p, ws, 1024), "code size between 1 and 16"), "code = 0 with a box term");
    expect(refused(call(4, 1, 17, 0, 0, p, p, p, 0, 0, 0, p, ws, 1024), "code size between 1 and 16"), "code = 17");
    expect(refused(call(4, 1, 8, p, 0, 0, 0, 0, 0, 0, 0, p, ws, 1024), "part_preds and part_labels come together"), "part_preds alone");
    expect(refused(call(4, 1, 8, 0, 0, p, 0, p, 0, 0, 0, p, ws, 1024), "come together"), "box_preds without box_labels");
    expect(refused(call(4, 1, 8, 0, 0, p, p, 0, 0, 0, 0, p, ws, 1024), "come together"), "box_preds without code_weights");
    expect(refused(call(4, 1, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, ws, 1024), "NULL or unaligned buffer"), "no table");
    expect(refused(call(4, 1, 8, 0, 0, 0, 0, 0, 0, 0, 0, p, 0, 1024), "NULL or unaligned buffer"), "no workspace");
    expect(refused(call(4, 1, 8, 0, 0, 0, 0, 0, 0, 0, 0, p, (char *)ws + 1, 1024), "NULL or unaligned buffer"), "unaligned workspace");
    expect(refused(call(4, 1, 8, 0, 0, 0, 0, 0, 0, 0, 0, p, ws, 511), "workspace smaller"), "workspace one byte short");
    expect(refused(call(4, 1, 8, 0, 0, p, p, p, p, 0, 0, p, ws, 1024), "gradient buffers come together"), "grad_cls without grad_box");
    expect(refused(call(4, 1, 8, 0, 0, 0, 0, 0, p, p, 0, p, ws, 1024), "gradient buffers come together"), "grad_part without a part term");
    expect(refused(call(4, 1, 8, 0, 0, 0, 0, 0, 0, 0, p, p, ws, 1024), "gradient buffers come together"), "grad_box without grad_cls");
    expect(refused(modest_point_loss(4, 1, 8, nullptr, p, 0, 0, 0, 0, 0, 0, 0.1f, 1.f, 1.f, 1.f, 0, 0, 0, p, ws, 1024, nullptr), "NULL buffer"),
           "no cls_preds");

    expect(refused(modest_point_loss_backward(-1, 0, 0, p, 0, 0, p, nullptr), "negative size"), "backward: a negative size");
    expect(refused(modest_point_loss_backward(max_rows * 32 + 1, 0, 0, p, 0, 0, p, nullptr), "more gradient elements"), "backward: too many");
    expect(refused(modest_point_loss_backward(4, 0, 0, nullptr, 0, 0, p, nullptr), "NULL buffer"), "backward: no buffer");
    expect(refused(modest_point_loss_backward(4, 0, 0, p, 0, 0, nullptr, nullptr), "NULL upstream"), "backward: no upstream");
    expect(modest_point_loss_backward(0, 0, 0, 0, 0, 0, 0, nullptr) == 0, "backward: nothing to scale is fine");
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
