// Stand-alone driver of the host-side checks of the box decoding (include/modest_hip.h, "a37"): every argument refusal of
// modest_anchor_decode / modest_point_decode / modest_roi_decode, and the calls that have nothing to do.  A refused call launches
// nothing, so the program needs no GPU; it is meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Imodest_amd/csrc tools/box_decode_host_check.cpp modest_amd/csrc/box_decode.hip \
//         -o box_decode_host_check && ./box_decode_host_check
//
// box_decode.hip needs nothing of the library but its error text, which csrc/ctx.hip keeps together with the context; the two
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
    const int64_t max_rows = modest_box_decode_max_rows();
    expect(max_rows == ((int64_t)1 << 31) - 1, "max_rows is 2^31 - 1");
    // host memory stands in for device memory: a refused call never touches it
    alignas(256) static float buf[256];
    float *p = buf;
    float *odd = reinterpret_cast<float *>(reinterpret_cast<char *>(buf) + 2);

    auto anchor = [&](int batch, int64_t n, int code, int sincos, const float *box, const float *anc, const float *dir, int bins,
                      float *out) { return modest_anchor_decode(batch, n, code, sincos, box, anc, dir, bins, 0.78f, 0.f, out, nullptr); };
    expect(refused(anchor(-1, 4, 7, 0, p, p, 0, 0, p), "batch >= 0"), "anchor: batch = -1");
    expect(refused(anchor(1, -1, 7, 0, p, p, 0, 0, p), "batch >= 0"), "anchor: n_anchors = -1");
    expect(refused(anchor(1, max_rows + 1, 7, 0, p, p, 0, 0, p), "batch >= 0"), "anchor: n_anchors = 2^31");
    expect(refused(anchor(2, (int64_t)1 << 30, 7, 0, p, p, 0, 0, p), "batch * n_anchors at most"), "anchor: 2 * 2^30 rows");
    expect(refused(anchor(INT32_MAX, max_rows, 7, 0, p, p, 0, 0, p), "batch * n_anchors at most"), "anchor: INT_MAX * (2^31 - 1) rows");
    expect(refused(anchor(1, 4, 6, 0, p, p, 0, 0, p), "code size between"), "anchor: code = 6");
    expect(refused(anchor(1, 4, 7, 1, p, p, 0, 0, p), "code size between"), "anchor: code = 7 with sincos");
    expect(refused(anchor(1, 4, 17, 0, p, p, 0, 0, p), "code size between"), "anchor: code = 17");
    expect(refused(anchor(1, 4, 17, 1, p, p, 0, 0, p), "code size between"), "anchor: code = 17 with sincos");
    expect(refused(anchor(1, 4, 7, 0, p, p, p, 0, p), "bins between 1 and 8"), "anchor: bins = 0 with a direction classifier");
    expect(refused(anchor(1, 4, 7, 0, p, p, p, 9, p), "bins between 1 and 8"), "anchor: bins = 9");
    expect(refused(anchor(1, 4, 7, 0, 0, p, 0, 0, p), "NULL buffer"), "anchor: no box_preds");
    expect(refused(anchor(1, 4, 7, 0, p, 0, 0, 0, p), "NULL buffer"), "anchor: no anchors");
    expect(refused(anchor(1, 4, 7, 0, p, p, 0, 0, 0), "NULL buffer"), "anchor: no output");
    expect(refused(anchor(1, 4, 7, 0, odd, p, 0, 0, p), "unaligned buffer"), "anchor: unaligned box_preds");
    expect(refused(anchor(1, 4, 7, 0, p, p, odd, 2, p), "unaligned buffer"), "anchor: unaligned dir_cls_preds");
    expect(anchor(0, 4, 7, 0, 0, 0, 0, 0, 0) == 0 && anchor(3, 0, 16, 0, 0, 0, 0, 0, 0) == 0, "anchor: nothing to decode is fine");

    auto point = [&](int64_t n, int code, int k, const float *box, const float *pts, int64_t stride, const float *cls,
                     const float *mean, float *out) { return modest_point_decode(n, code, k, box, pts, stride, cls, mean, out, nullptr); };
    expect(refused(point(-1, 8, 3, p, p, 3, p, 0, p), "n_rows between"), "point: n_rows = -1");
    expect(refused(point(max_rows + 1, 8, 3, p, p, 3, p, 0, p), "n_rows between"), "point: n_rows = 2^31");
    expect(refused(point(INT64_MAX, 8, 3, p, p, 3, p, 0, p), "n_rows between"), "point: n_rows = INT64_MAX");
    expect(refused(point(4, 7, 3, p, p, 3, p, 0, p), "code size between 8 and 16"), "point: code = 7");
    expect(refused(point(4, 17, 3, p, p, 3, p, 0, p), "code size between 8 and 16"), "point: code = 17");
    expect(refused(point(4, 8, 0, p, p, 3, p, 0, p), "num_class between 1 and 32"), "point: num_class = 0");
    expect(refused(point(4, 8, 33, p, p, 3, p, 0, p), "num_class between 1 and 32"), "point: num_class = 33");
    expect(refused(point(4, 8, 3, p, p, 2, p, 0, p), "at least 3"), "point: a row stride of 2");
    expect(refused(point(4, 8, 3, 0, p, 3, p, 0, p), "NULL buffer"), "point: no box_preds");
    expect(refused(point(4, 8, 3, p, 0, 3, p, 0, p), "NULL buffer"), "point: no points");
    expect(refused(point(4, 8, 3, p, p, 3, 0, 0, p), "NULL buffer"), "point: no cls_preds");
    expect(refused(point(4, 8, 3, p, p, 3, p, odd, p), "unaligned buffer"), "point: unaligned mean_size");
    expect(point(0, 8, 3, 0, 0, 3, 0, 0, 0) == 0, "point: nothing to decode is fine");

    expect(refused(modest_roi_decode(-1, 7, p, p, p, nullptr), "n_rows between"), "roi: n_rows = -1");
    expect(refused(modest_roi_decode(max_rows + 1, 7, p, p, p, nullptr), "n_rows between"), "roi: n_rows = 2^31");
    expect(refused(modest_roi_decode(4, 6, p, p, p, nullptr), "code size between 7 and 16"), "roi: code = 6");
    expect(refused(modest_roi_decode(4, 17, p, p, p, nullptr), "code size between 7 and 16"), "roi: code = 17");
    expect(refused(modest_roi_decode(4, 7, 0, p, p, nullptr), "NULL buffer"), "roi: no rois");
    expect(refused(modest_roi_decode(4, 7, p, 0, p, nullptr), "NULL buffer"), "roi: no box_preds");
    expect(refused(modest_roi_decode(4, 7, p, p, 0, nullptr), "NULL buffer"), "roi: no output");
    expect(refused(modest_roi_decode(4, 7, p, p, odd, nullptr), "unaligned buffer"), "roi: unaligned output");
    expect(modest_roi_decode(0, 7, 0, 0, 0, nullptr) == 0, "roi: nothing to decode is fine");
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
