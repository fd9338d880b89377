"""The arithmetic contract of csrc/pillar_vfe.hip restated in numpy, operation by operation, and the
exact (float64) value of the same chain with a DERIVED float32 error bound per element.

THE CONTRACT.  float32, one rounding per operation in the written order; / and sqrt correctly rounded.
  features   sum_j = v[0][j] + v[1][j] + ... over ALL S slots in slot order (j = 0..2); mean_j = sum_j / float32(num);
             cluster v_j - mean_j; centre v_0 - (float32(coord_x) * vx + xoff) with vx = float32(voxel_x) and xoff =
             float32(voxel_x / 2 + range[0]) (y with coords[:, 2], z with coords[:, 1]); distance sqrt((x*x + y*y) + z*z);
             order [v or v[3:], cluster, centre, distance]; then every feature TIMES float32(int(num) > s): num = 0 gives NaN
             features in every slot (0 / 0, then NaN * 0).
  linear     x = f_0 * W[c, 0], then + f_k * W[c, k] for k = 1 .. K - 1.
  statistics (training) over all N = P * S rows, padded rows included, in float64: sum x, sum x*x, sum x*f_k per channel and
             sum f_k (the products are exact in float64), added over THE TREE: a run of RUN consecutive pillars in pillar order
             then slot order, GROUP runs in ascending order, the groups in ascending order, each sum started at +0.0.
             mean = sum x / N; var = max(sum x*x / N - mean*mean, 0) (a NaN kept); invstd = 1 / sqrt(var + eps); mean32, invstd32
             their float32.  running = (1 - m) * running + m * new in float64, rounded to float32, with var * N / (N - 1) for
             running_var; m = momentum, or 1 / (tracked + 1) for momentum None; tracked += 1.
             eval: mean32 = running_mean, invstd32 = float32(1 / sqrt(float64(running_var) + eps)); nothing changes.
  normalise  xhat = (x - mean32) * invstd32; t = xhat * gamma + beta; y = t where t > 0 or t is a NaN, else +0;
             out[p, c] = max over ALL S slots, the winner its FIRST slot; a NaN counts as the maximum, the first NaN wins.
  backward   dy = g where out > 0 else 0, at the winner's slot; over the same tree (pillars only) in float64: dbeta = sum dy,
             dgamma = sum dy * xhat, A[c, k] = sum dy * f_k (exact products); with g = gamma, mean = float64(mean32), invstd =
             float64(invstd32):  dW[c, k] = invstd * (((g * A) - ((g * dbeta) / N) * Sf_k) - (((g * dgamma) / N) * invstd) *
             (Sxf[c, k] - mean * Sf_k)), rounded to float32 like dgamma and dbeta.
  TIES.  The first slot of the maximum wins.  No tie changes out, dW, dgamma or dbeta: tied slots hold the same y, so out is
  the same; a tie at y = 0 has out = 0 and therefore dy = 0, so it carries no gradient whichever slot is named; two padded slots
  (s >= num) hold the same features (f = v * 0 with the same v = 0 rows of a voxeliser, or exactly the masked zeros), hence
  the same x and xhat, and contribute identically.  Distinct real points that tie at a positive y bit for bit are the one case
  where the named slot matters for dW; the first is named, here and in the kernel.
  scatter    canvas (B, C, ny, nx) zeros, then canvas[b, c, y, x] = feat[p, c]; a row whose b, z, y or x is out of range
             (nz = 1) is skipped; backward grad_feat[p, c] = grad_canvas[b, c, y, x], zeros for a skipped row.

THE BOUND (`exact`).  Every quantity is also evaluated in float64 ("exact": its own error is 2^-29 of float32's), and a bound
on |any float32 evaluation - exact| is carried along per element, first-order terms with u = 2^-24 and gamma_n = n u / (1 - n
u) for an n-term sum in ANY order, so that it holds for the reference's torch kernels as for this restatement.  See the
comments in `exact`.  The gradients' bound needs the winners to be decided beyond the error of y (`margins`); a scene where
that does not hold is refused.
"""
import json

import numpy as np

F, D = np.float32, np.float64
U = 2.0 ** -24
RUN, GROUP = 32, 64          # ops.pillar_vfe_run() / ops.pillar_vfe_group(): the GPU tests check that they are these
XYZ, CLUSTER, CENTER, DIST = 1, 2, 4, 8
WRONG = ("unbiased_norm", "eps", "no_pad_stats", "no_pad_max", "no_mask", "biased_running")
FIELDS = ("voxels", "num", "coords", "W", "gamma", "beta", "running_mean", "running_var")


def gam(n):
    return n * U / (1.0 - n * U)


def parts_of(use_abs=True, with_dist=False):
    return CLUSTER | CENTER | (XYZ if use_abs else 0) | (DIST if with_dist else 0)


def n_features(Cp, parts):
    return (Cp if parts & XYZ else Cp - 3) + (3 if parts & CLUSTER else 0) + (3 if parts & CENTER else 0) + (1 if parts & DIST else 0)


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == F:
        b = a.view(np.uint32).copy()
        b[np.isnan(a)] = 0x7FC00000          # every NaN counts as one value
        return b
    if a.dtype == D:
        b = a.view(np.uint64).copy()
        b[np.isnan(a)] = 0x7FF8000000000000
        return b
    return a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def report(got, want, label=""):
    """'' where got equals want bit for bit in every element, else the first elements that differ"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{label} shape / dtype {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    bad = np.argwhere(bits(got) != bits(want))
    if not len(bad):
        return ""
    rows = [f"{label} {len(bad)} of {got.size} elements differ"]
    for at in bad[:6]:
        at = tuple(int(i) for i in at)
        rows.append(f"  {at}: got {got[at]!r}, want {want[at]!r}")
    return "\n".join(rows)


def bound_report(got, value, bound, label=""):
    """-> ('' or what leaves the bound, the largest |got - value| / bound); non-finite exact values must match as patterns"""
    got = np.asarray(got, D).reshape(value.shape)
    fin = np.isfinite(value) & np.isfinite(bound)
    if not np.array_equal(np.isnan(got[~fin]), np.isnan(value[~fin])):
        return f"{label} NaN pattern differs where the exact value is not finite", np.inf
    if not fin.any():
        return "", 0.0
    err = np.abs(got[fin] - value[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound[fin])
    worst = float(ratio.max())
    if worst <= 1.0:
        return "", worst
    i = int(np.argmax(ratio))
    return f"{label} element {i} of the finite ones: got {got[fin][i]!r}, exact {value[fin][i]!r}, bound {bound[fin][i]:.3e}, ratio {worst:.3f}", worst


def pattern_report(a, b, label=""):
    a, b = np.asarray(a), np.asarray(b).reshape(np.asarray(a).shape)
    for name, fn in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        if not np.array_equal(fn(a), fn(b)):
            return f"{label} the {name} pattern differs"
    return ""


def seq_sum(a, axis=0):
    """the sum along `axis` in ascending order from +0.0, one rounding per addition (cumsum is sequential)"""
    a = np.moveaxis(np.asarray(a), axis, 0)
    return np.cumsum(np.concatenate([np.zeros((1,) + a.shape[1:], a.dtype), a]), axis=0)[-1]


def tree_total(partials):
    """(runs, ...) float64 partials -> their total over the groups' tree"""
    runs = partials.shape[0]
    groups = (runs + GROUP - 1) // GROUP
    pad = np.zeros((groups * GROUP,) + partials.shape[1:], D)
    pad[:runs] = partials
    return seq_sum(seq_sum(pad.reshape((groups, GROUP) + partials.shape[1:]), axis=1), axis=0)


def to_int(num):
    """torch's .int() of the pillar's count"""
    if num.dtype == F:
        with np.errstate(invalid="ignore"):
            return np.where(np.isnan(num), 0, np.clip(np.trunc(num.astype(D)), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
    return num.astype(np.int32).astype(np.int64)


def features(case, wrong=None):
    """-> (P, S, K) float32"""
    v, num, coords, parts = case["voxels"], case["num"], case["coords"], case["parts"]
    P, S, Cp = v.shape
    with np.errstate(all="ignore"):
        total = v[:, 0, :3].copy()
        for s in range(1, S):
            total = total + v[:, s, :3]
        mean = total / num.astype(F)[:, None]
        cols = [v if parts & XYZ else v[:, :, 3:]]
        if parts & CLUSTER:
            cols.append(v[:, :, :3] - mean[:, None, :])
        if parts & CENTER:
            cf = coords.astype(F)
            centre = np.stack([cf[:, 3 - j] * F(case["voxel_size"][j]) + F(case["offsets"][j]) for j in range(3)], axis=1)
            cols.append(v[:, :, :3] - centre[:, None, :])
        if parts & DIST:
            x, y, z = v[:, :, 0], v[:, :, 1], v[:, :, 2]
            cols.append(np.sqrt((x * x + y * y) + z * z)[:, :, None])
        f = np.concatenate(cols, axis=2)
        if wrong != "no_mask":
            f = f * (to_int(num)[:, None] > np.arange(S)[None, :]).astype(F)[:, :, None]
    assert f.dtype == F and f.shape == (P, S, n_features(Cp, parts))
    return f


def linear(f, W):
    """f (..., K), W (C, K) -> x (..., C) float32 in the kernel's order.  Large inputs go through torch's CPU kernels, which
    round each product and each sum as numpy does (IEEE, nothing fused) on several threads."""
    if f.size * W.shape[0] >= 1 << 22:
        import torch
        ft, Wt = torch.from_numpy(np.ascontiguousarray(f)), torch.from_numpy(np.ascontiguousarray(W))
        x = ft[..., None, 0] * Wt[:, 0]
        for k in range(1, W.shape[1]):
            x += ft[..., None, k] * Wt[:, k]
        return x.numpy()
    with np.errstate(all="ignore"):
        x = f[..., None, 0] * W[..., 0]
        for k in range(1, W.shape[-1]):
            x = x + f[..., None, k] * W[..., k]
    return x


def keep_positive(t):
    return np.where((t > 0) | np.isnan(t), t, 0.0)


def forward_sums(f, W):
    """the float64 sums of a training forward over the tree -> [Sx (C), Sxx (C), Sxf (K, C), Sf (K)] flat"""
    P, S, K = f.shape
    C = W.shape[0]
    runs = (P + RUN - 1) // RUN
    fp = np.zeros((runs * RUN, S, K), F)
    fp[:P] = f
    live = (np.arange(runs * RUN) < P).reshape(runs, RUN)
    fp = fp.reshape(runs, RUN, S, K)
    sx, sxx, sxf, sf = np.zeros((runs, C)), np.zeros((runs, C)), np.zeros((runs, K, C)), np.zeros((runs, K))
    tmp = np.empty((runs, K, C))
    big = tmp.size >= 1 << 18
    if big:                                   # the same IEEE products and sums on several threads
        import torch
        sxf_t = torch.from_numpy(sxf)
    with np.errstate(all="ignore"):
        for r in range(min(RUN, P)):
            on = live[:, r]
            xr = linear(np.ascontiguousarray(fp[:, r]), W).astype(D)          # (runs, S, C)
            fr = fp[:, r].astype(D)
            if not on.all():                                                  # a pillar past the end adds +0.0
                xr, fr = np.where(on[:, None, None], xr, 0.0), np.where(on[:, None, None], fr, 0.0)
            for s in range(S):
                xd, fd = np.ascontiguousarray(xr[:, s]), np.ascontiguousarray(fr[:, s])
                sx += xd
                sxx += xd * xd
                if big:                     # one pass: the product is exact, so fused or not it is rounded once, in the sum
                    sxf_t.addcmul_(torch.from_numpy(xd)[:, None, :], torch.from_numpy(fd)[:, :, None])
                else:
                    np.multiply(xd[:, None, :], fd[:, :, None], out=tmp)
                    sxf += tmp
                sf += fd
    return np.concatenate([tree_total(a).reshape(-1) for a in (sx, sxx, sxf, sf)])


def apply_pass(f, W, mean32, invstd32, gamma, beta, num=None, chunk=2048):
    """-> out (P, C) float32, winner (P, C) uint8; `num`: the wrong variant that leaves padded slots out of the maximum"""
    P, S, K = f.shape
    C = W.shape[0]
    out, win = np.empty((P, C), F), np.empty((P, C), np.uint8)
    with np.errstate(all="ignore"):
        for a in range(0, P, chunk):
            x = linear(f[a:a + chunk], W)
            xhat = (x - mean32) * invstd32
            t = xhat * gamma + beta
            y = np.where((t > 0) | np.isnan(t), t, F(0)).astype(F)
            if num is not None:
                y = np.where((to_int(num[a:a + chunk])[:, None] > np.arange(S)[None, :])[:, :, None], y, F(-np.inf))
            w = np.argmax(y, axis=1)                     # the first maximum; a NaN counts as the maximum, the first NaN wins
            out[a:a + chunk] = np.take_along_axis(y, w[:, None, :], axis=1)[:, 0, :]
            win[a:a + chunk] = w
    return out, win


def restate(case, wrong=None):
    """one forward call -> dict(out, winner, sums, stat, running_mean, running_var, tracked); training per case['training']"""
    f = features(case, wrong)
    W, gamma, beta = case["W"], case["gamma"], case["beta"]
    P, S, K = f.shape
    C = W.shape[0]
    eps = 1e-5 if wrong == "eps" else float(case["eps"])
    rm, rv = case.get("running_mean"), case.get("running_var")
    res = {"running_mean": None if rm is None else rm.copy(), "running_var": None if rv is None else rv.copy(),
           "tracked": case.get("tracked", 0), "sums": None, "stat": None}
    with np.errstate(all="ignore"):
        if case["training"]:
            sums = forward_sums(f, W)
            N = float(P * S)
            if wrong == "no_pad_stats":
                N = float(np.minimum(np.maximum(to_int(case["num"]), 0), S).sum())
            mean = sums[:C] / N
            var = keep_positive(sums[C:2 * C] / N - mean * mean)
            used = var * N / (N - 1.0) if wrong == "unbiased_norm" else var
            invstd = 1.0 / np.sqrt(used + eps)
            mean32, invstd32 = mean.astype(F), invstd.astype(F)
            res["sums"], res["stat"] = sums, np.stack([mean32, invstd32])
            if rm is not None:
                m = 1.0 / (res["tracked"] + 1) if case["momentum"] is None else float(case["momentum"])
                unbiased = var if wrong == "biased_running" else var * N / (N - 1.0)
                res["running_mean"] = ((1.0 - m) * rm.astype(D) + m * mean).astype(F)
                res["running_var"] = ((1.0 - m) * rv.astype(D) + m * unbiased).astype(F)
                res["tracked"] = res["tracked"] + 1
        else:
            mean32, invstd32 = rm, (1.0 / np.sqrt(rv.astype(D) + eps)).astype(F)
    res["out"], res["winner"] = apply_pass(f, W, mean32, invstd32, gamma, beta, case["num"] if wrong == "no_pad_max" else None)
    if not case["training"]:
        res["winner"] = None
    res["features"] = f
    return res


def restate_steps(case, wrong=None):
    """case['steps'] forward calls in a row on the same inputs, the running buffers carried -> the last call's dict"""
    cur = dict(case)
    for _ in range(int(case.get("steps", 1))):
        res = restate(cur, wrong)
        cur["running_mean"], cur["running_var"], cur["tracked"] = res["running_mean"], res["running_var"], res["tracked"]
    return res


def restate_backward(case, fwd, grad):
    """-> dW (C, K), dgamma (C,), dbeta (C,) float32 from a training forward's dict"""
    f, W, gamma = fwd["features"], case["W"], case["gamma"]
    P, S, K = f.shape
    C = W.shape[0]
    mean32, invstd32 = fwd["stat"]
    runs = (P + RUN - 1) // RUN
    with np.errstate(all="ignore"):
        fw = f[np.arange(P)[:, None], fwd["winner"].astype(np.int64), :]                    # (P, C, K)
        xhat = (linear_rows(fw, W) - mean32) * invstd32
        dy = np.where(fwd["out"] > 0, grad, F(0)).astype(D)
        pad = lambda a: np.concatenate([a, np.zeros((runs * RUN - P,) + a.shape[1:], a.dtype)]).reshape((runs, RUN) + a.shape[1:])   # noqa: E731
        on = pad(np.ones(P, bool))
        z = lambda a: np.where(on.reshape(on.shape + (1,) * (a.ndim - 2)), a, 0.0)         # noqa: E731
        db = tree_total(seq_sum(z(pad(dy)), axis=1))
        dg = tree_total(seq_sum(z(pad(dy * xhat.astype(D))), axis=1))
        A = tree_total(seq_sum(z(pad(dy[:, :, None] * fw.astype(D))), axis=1))             # (C, K)
        sums = fwd["sums"]
        sxf, sf = sums[2 * C:2 * C + K * C].reshape(K, C).T, sums[2 * C + K * C:]
        N = float(P * S)
        g, mean, invstd = gamma.astype(D)[:, None], mean32.astype(D)[:, None], invstd32.astype(D)[:, None]
        t1 = g * A
        t2 = ((g * db[:, None]) / N) * sf[None, :]
        t3 = (((g * dg[:, None]) / N) * invstd) * (sxf - mean * sf[None, :])
        dW = invstd * ((t1 - t2) - t3)
    return dW.astype(F), dg.astype(F), db.astype(F)


def linear_rows(fw, W):
    """fw (P, C, K): the features each channel's winner holds -> x (P, C)"""
    with np.errstate(all="ignore"):
        x = fw[..., 0] * W[None, :, 0]
        for k in range(1, W.shape[1]):
            x = x + fw[..., k] * W[None, :, k]
    return x


def in_range(coords, B, ny, nx):
    c = coords.astype(D)
    with np.errstate(invalid="ignore"):
        return (c[:, 0] >= 0) & (c[:, 0] < B) & (c[:, 1] >= 0) & (c[:, 1] < 1) & (c[:, 2] >= 0) & (c[:, 2] < ny) & (c[:, 3] >= 0) & (c[:, 3] < nx)


def scatter(feat, coords, B, ny, nx):
    P, C = feat.shape
    canvas = np.zeros((B, C, ny, nx), F)
    ok = in_range(coords, B, ny, nx)
    c = np.where(ok[:, None], np.nan_to_num(coords.astype(D)), 0).astype(np.int64)
    canvas[c[ok, 0], :, c[ok, 2], c[ok, 3]] = feat[ok]
    return canvas


def scatter_backward(grad_canvas, coords):
    B, C, ny, nx = grad_canvas.shape
    ok = in_range(coords, B, ny, nx)
    c = np.where(ok[:, None], np.nan_to_num(coords.astype(D)), 0).astype(np.int64)
    grad = np.zeros((len(coords), C), F)
    grad[ok] = grad_canvas[c[ok, 0], :, c[ok, 2], c[ok, 3]]
    return grad


# ------------------------------------------------------------------------------------------------ exact values and their bound
def exact(case, grad=None):
    """-> {name: (exact float64 value, bound on |a float32 evaluation - exact|)} for out, running_mean, running_var and -- with
    `grad` (P, C), in training mode -- dW, dgamma, dbeta; 'margin': '' or why the winners are not decided beyond the bound.
    Finite inputs with num >= 1 only."""
    v, num, coords, parts = case["voxels"].astype(D), case["num"].astype(D), case["coords"].astype(D), case["parts"]
    W, gamma, beta = case["W"].astype(D), case["gamma"].astype(D), case["beta"].astype(D)
    P, S, Cp = v.shape
    C, K = W.shape
    N = float(P * S)
    eps = float(case["eps"])
    mask = (np.trunc(num)[:, None] > np.arange(S)[None, :]).astype(D)
    # features: value and error.  The inputs are exact.
    a3 = np.abs(v[:, :, :3])
    mean = v[:, :, :3].sum(1) / num[:, None]
    e_mean = (gam(S - 1) * a3.sum(1) / num[:, None] + U * np.abs(mean)) * (1 + gam(2))        # an S-term sum in any order, one division
    cols, errs = [v if parts & XYZ else v[:, :, 3:]], [np.zeros_like(v if parts & XYZ else v[:, :, 3:])]
    if parts & CLUSTER:
        fc = v[:, :, :3] - mean[:, None, :]
        cols.append(fc)
        errs.append(e_mean[:, None, :] + U * (np.abs(fc) + e_mean[:, None, :]))               # the subtrahend's error, one rounding
    if parts & CENTER:
        vs = np.array([D(F(t)) for t in case["voxel_size"]])
        off = np.array([D(F(t)) for t in case["offsets"]])
        prod = coords[:, [3, 2, 1]] * vs[None, :]
        centre = prod + off[None, :]
        e_c = U * np.abs(prod) + U * (np.abs(centre) + U * np.abs(prod))                       # a product and a sum
        fcen = v[:, :, :3] - centre[:, None, :]
        cols.append(fcen)
        errs.append(e_c[:, None, :] + U * (np.abs(fcen) + e_c[:, None, :]))
    if parts & DIST:
        d = np.sqrt((v[:, :, :3] ** 2).sum(2))
        cols.append(d[:, :, None])
        errs.append((3.0 * U * d)[:, :, None] * (1 + gam(4)))      # radicand of positive terms: 3 u relative, halved by sqrt, + u
    f = np.concatenate(cols, 2) * mask[:, :, None]
    e_f = np.concatenate(errs, 2) * mask[:, :, None]
    # linear: a K-term dot product in any order on perturbed features
    x = np.einsum("psk,ck->psc", f, W)
    ax = np.einsum("psk,ck->psc", np.abs(f), np.abs(W))
    e_x = (np.einsum("psk,ck->psc", e_f, np.abs(W)) + gam(K) * ax) * (1 + gam(K))
    out = {}
    rm = None if case.get("running_mean") is None else case["running_mean"].astype(D)
    rv = None if case.get("running_var") is None else case["running_var"].astype(D)
    e_rm = None if rm is None else np.zeros(C)
    e_rv = None if rv is None else np.zeros(C)
    tracked = case.get("tracked", 0)
    if case["training"]:
        # mean of N rows summed in any order in float32, of perturbed x
        mu = x.sum((0, 1)) / N
        e_mu = (e_x.sum((0, 1)) / N + gam(N) * np.abs(x).sum((0, 1)) / N + U * np.abs(mu)) * (1 + gam(2))
        # var = sum x x / N - mean mean: both terms move with x's and the mean's error, and each is a float32 evaluation of its own
        # (the cancellation between them is paid in full: the bound is on the terms, not on their difference)
        m2 = (x * x).sum((0, 1)) / N
        var = np.maximum(m2 - mu * mu, 0.0)
        e_var = ((2 * np.abs(x) * e_x + e_x * e_x).sum((0, 1)) / N + 2 * np.abs(mu) * e_mu + e_mu * e_mu
                 + gam(N + 2) * (m2 + mu * mu) + U * var)
        for _ in range(int(case.get("steps", 1))):
            if rm is not None:
                m = 1.0 / (tracked + 1) if case["momentum"] is None else float(case["momentum"])
                unb = var * N / (N - 1.0)
                new_rm, new_rv = (1 - m) * rm + m * mu, (1 - m) * rv + m * unb
                e_rm = (1 - m) * e_rm + m * e_mu + 3 * U * (np.abs((1 - m) * rm) + np.abs(m * mu)) + U * np.abs(new_rm)
                e_rv = ((1 - m) * e_rv + m * (e_var * N / (N - 1.0) + 2 * U * unb) + 3 * U * (np.abs((1 - m) * rv) + np.abs(m * unb))
                        + U * np.abs(new_rv))
                rm, rv, tracked = new_rm, new_rv, tracked + 1
        lo = np.maximum(var - e_var, 0.0) + eps
    else:
        mu, e_mu, var, e_var = rm, np.zeros(C), rv, np.zeros(C)
        lo = var + eps
    invstd = 1.0 / np.sqrt(var + eps)
    e_is = 0.5 * e_var * lo ** -1.5 + 3 * U / np.sqrt(lo)                                      # the slope at the interval's low end
    # xhat, y in either association: (x - mean) invstd gamma + beta, or x (invstd gamma) + (beta - mean invstd gamma)
    xc = x - mu
    xhat = xc * invstd
    e_xhat = ((e_x + e_mu + U * np.abs(xc)) * (invstd + e_is) + np.abs(xc) * e_is + U * np.abs(xhat)) * (1 + gam(3))
    t = xhat * gamma + beta
    e_t = (np.abs(gamma) * e_xhat + 4 * U * (np.abs(x) + np.abs(mu)) * np.abs(invstd * gamma) + 2 * U * np.abs(beta) + U * np.abs(t)) * (1 + gam(3))
    y = np.maximum(t, 0.0)
    w = np.argmax(y, axis=1)                                                                  # (P, C)
    best = np.take_along_axis(y, w[:, None, :], 1)[:, 0, :]
    out["out"] = (best, e_t.max(axis=1))                     # |max of perturbed - max of exact| <= the largest perturbation
    if rm is not None and case["training"]:
        out["running_mean"], out["running_var"] = (rm, e_rm), (rv, e_rv)
    out["margin"] = ""
    if grad is not None and case["training"]:
        # The winner must be decided: every slot that is not the winner's twin (the same feature row, as padded slots are) lies
        # below it by more than both errors, and a winner at a positive y lies above zero by more than its error.
        tw = np.take_along_axis(t, w[:, None, :], 1)
        e_w = np.take_along_axis(e_t, w[:, None, :], 1)
        fw = f[np.arange(P)[:, None], w, :]                                                   # (P, C, K)
        twin = (f[:, :, None, :] == fw[:, None, :, :]).all(3)                                 # (P, S, C)
        close = ~twin & (np.maximum(tw, 0.0) - np.maximum(t, 0.0) <= e_w + e_t) & ((tw > -e_w) | (t > -e_t))
        if close.any():
            out["margin"] = f"{int(close.sum())} slots lie within the error of their pillar's maximum"
        edge = np.abs(tw[:, 0, :]) <= e_w[:, 0, :]
        if edge.any():
            out["margin"] += f" {int(edge.sum())} winners lie within their error of zero"
        g = grad.astype(D)
        dy = np.where(best > 0, g, 0.0)                                                       # exact: g is an input
        xw = np.take_along_axis(xhat, w[:, None, :], 1)[:, 0, :]
        e_xw = np.take_along_axis(e_xhat, w[:, None, :], 1)[:, 0, :]
        db = dy.sum(0)
        e_db = gam(P) * np.abs(dy).sum(0) + U * np.abs(db)
        dg = (dy * xw).sum(0)
        e_dg = (np.abs(dy) * e_xw).sum(0) + gam(P + 1) * np.abs(dy * xw).sum(0) + U * np.abs(dg)
        out["dbeta"], out["dgamma"] = (db, e_db), (dg, e_dg)
        # dW the reference's way: dx = a (dyfull - b - xhat d) per row, a = invstd gamma, b = dbeta / N, d = dgamma / N, then
        # dW = sum over the N rows of dx f_k in any order
        dyf = np.zeros((P, S, C))
        np.put_along_axis(dyf, w[:, None, :], dy[:, None, :], 1)
        a, b, d = invstd * gamma, db / N, dg / N
        e_a = np.abs(gamma) * e_is + U * np.abs(a)
        e_b, e_d = e_db / N + U * np.abs(b), e_dg / N + U * np.abs(d)
        inner = dyf - b - xhat * d
        dx = a * inner
        e_dx = (e_a * np.abs(inner) + (np.abs(a) + e_a) * (e_b + e_xhat * (np.abs(d) + e_d) + np.abs(xhat) * e_d)
                + 4 * U * (np.abs(a) + e_a) * (np.abs(dyf) + np.abs(b) + np.abs(xhat * d)))
        dW = np.einsum("psc,psk->ck", dx, f)
        e_dW = (np.einsum("psc,psk->ck", e_dx, np.abs(f) + e_f) + np.einsum("psc,psk->ck", np.abs(dx), e_f)
                + gam(N) * np.einsum("psc,psk->ck", np.abs(dx), np.abs(f)) + U * np.abs(dW))
        out["dW"] = (dW, e_dW)
    return out


# ------------------------------------------------------------------------------------------------ cases
def make_case(seed, P, S, Cp=4, C=64, use_abs=True, with_dist=False, training=True, steps=1, B=2, ny=5, nx=6, parts=None,
              num=None, eps=1e-3, momentum=0.01, num_dtype=F, coord_dtype=F, fresh=None):
    """a case with P pillars in distinct cells of a (B, ny, nx) grid; `num`: the counts, by default a mix of 1, S and between"""
    rng = np.random.default_rng(seed)
    parts = parts_of(use_abs, with_dist) if parts is None else parts
    K = n_features(Cp, parts)
    voxel_size, rng_lo = (0.25, 0.25, 8.0), (-0.75, -0.625, -3.0)
    cells = rng.permutation(B * ny * nx)[:P] if P <= B * ny * nx else np.arange(P)
    cells = np.sort(cells)
    b, y, x = cells // (ny * nx), (cells // nx) % ny, cells % nx
    coords = np.stack([b, np.zeros_like(b), y, x], 1)
    if num is None:
        num = rng.integers(1, S + 1, P)
        num[::3] = S
        num[1::4] = 1
    num = np.broadcast_to(np.asarray(num), (P,)).copy()
    v = np.zeros((P, S, Cp), F)
    lo = np.array([rng_lo[0] + x * voxel_size[0], rng_lo[1] + y * voxel_size[1], np.full(P, rng_lo[2])], D).T
    pts = lo[:, None, :] + rng.random((P, S, 3)) * np.array(voxel_size)[None, None, :]
    v[:, :, :3] = pts.astype(F)
    v[:, :, 3:] = rng.random((P, S, Cp - 3)).astype(F)
    v *= (np.clip(num, 0, S)[:, None] > np.arange(S)[None, :])[:, :, None]                   # a voxeliser leaves padded slots zero
    case = dict(voxels=v, num=num.astype(num_dtype), coords=coords.astype(coord_dtype), parts=int(parts),
                voxel_size=voxel_size, offsets=tuple(voxel_size[i] / 2 + rng_lo[i] for i in range(3)),
                W=(rng.standard_normal((C, K)) * 0.5).astype(F), gamma=rng.uniform(0.5, 1.5, C).astype(F),
                beta=(rng.standard_normal(C) * 0.3).astype(F), eps=eps, momentum=momentum, training=bool(training), steps=int(steps),
                batch_size=B, ny=ny, nx=nx, tracked=0, seed=int(seed))
    fresh = training if fresh is None else fresh
    case["running_mean"] = np.zeros(C, F) if fresh else (rng.standard_normal(C) * 0.3).astype(F)
    case["running_var"] = np.ones(C, F) if fresh else rng.uniform(0.3, 1.2, C).astype(F)
    case["grad"] = rng.standard_normal((P, C)).astype(F)
    return case


_fill = {}


def grad_canvas_of(case):
    """the upstream gradient of the canvas: case['grad'] in the pillars' cells, a seeded fill elsewhere"""
    C = case["W"].shape[0]
    key = (case["seed"], case["batch_size"], C, case["ny"], case["nx"])
    if key not in _fill:                                                       # drawn once per shape, left unchanged
        _fill.clear()
        _fill[key] = np.random.default_rng(case["seed"] + 1000).standard_normal(key[1:], dtype=F)
    G = _fill[key].copy()
    ok = in_range(case["coords"], case["batch_size"], case["ny"], case["nx"])
    c = np.where(ok[:, None], np.nan_to_num(case["coords"].astype(D)), 0).astype(np.int64)
    G[c[ok, 0], :, c[ok, 2], c[ok, 3]] = case["grad"][ok]
    return G


def grad_feat_of(case):
    """what scatter_backward makes of grad_canvas_of(case): the recorded gradient, zeros for a row out of range"""
    ok = in_range(case["coords"], case["batch_size"], case["ny"], case["nx"])
    return np.where(ok[:, None], case["grad"], F(0)).astype(F)


CFG_KEYS = ("parts", "voxel_size", "offsets", "eps", "momentum", "training", "steps", "batch_size", "ny", "nx", "tracked", "seed")


def pack(name, case, rec):
    """-> {key: array} of one scene for the fixture"""
    out = {name + "_cfg": np.array(json.dumps({k: case[k] for k in CFG_KEYS}))}
    for k in FIELDS:
        out[f"{name}_{k}"] = case[k]
    for k, a in rec.items():
        out[f"{name}_rec_{k}"] = a
    return out


def scenes(npz):
    """the fixture -> [(name, case, recording)]"""
    res = []
    for name in json.loads(str(npz["scenes"])):
        case = json.loads(str(npz[name + "_cfg"]))
        case["voxel_size"], case["offsets"] = tuple(case["voxel_size"]), tuple(case["offsets"])
        for k in FIELDS:
            case[k] = npz[f"{name}_{k}"]
        rec = {k[len(name) + 5:]: npz[k] for k in npz if k.startswith(name + "_rec_")}
        case["grad"] = rec.get("grad_feat")          # the upstream gradient of the features is the recorded one
        if case["grad"] is None:                     # eval mode records none: a seeded one for the scatter's backward
            shape = (case["voxels"].shape[0], case["W"].shape[0])
            case["grad"] = np.random.default_rng(case["seed"] + 2000).standard_normal(shape, dtype=F)
        res.append((name, case, rec))
    return res


# ------------------------------------------------------------------------------------------------ stand-in modules (torch)
def bare_modules(case, device):
    """minimal stand-ins for PillarVFE and PointPillarScatter with our forward methods bound -> (vfe, scatter, batch_dict)"""
    import torch
    from torch import nn
    from modest_amd.utils import pillar_vfe as pv

    C, K = case["W"].shape

    class PFN(nn.Module):
        def __init__(self):
            super().__init__()
            self.use_norm = True
            self.linear = nn.Linear(K, C, bias=False)
            self.norm = nn.BatchNorm1d(C, eps=case["eps"], momentum=case["momentum"])

    class VFE(nn.Module):
        forward = pv.pillar_vfe_forward

        def __init__(self):
            super().__init__()
            self.pfn_layers = nn.ModuleList([PFN()])
            self.use_absolute_xyz, self.with_distance = bool(case["parts"] & XYZ), bool(case["parts"] & DIST)
            self.voxel_x, self.voxel_y, self.voxel_z = case["voxel_size"]
            self.x_offset, self.y_offset, self.z_offset = case["offsets"]

    class Scatter(nn.Module):
        forward = pv.pillar_scatter_forward

        def __init__(self):
            super().__init__()
            self.num_bev_features, self.nx, self.ny, self.nz = C, case["nx"], case["ny"], 1

    vfe, sc = VFE().to(device), Scatter().to(device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)                     # noqa: E731
    pfn = vfe.pfn_layers[0]
    with torch.no_grad():
        pfn.linear.weight.copy_(t(case["W"]))
        pfn.norm.weight.copy_(t(case["gamma"]))
        pfn.norm.bias.copy_(t(case["beta"]))
        pfn.norm.running_mean.copy_(t(case["running_mean"]))
        pfn.norm.running_var.copy_(t(case["running_var"]))
        pfn.norm.num_batches_tracked.fill_(int(case.get("tracked", 0)))
    vfe.train(case["training"])
    batch = {"voxels": t(case["voxels"]), "voxel_num_points": t(case["num"]), "voxel_coords": t(case["coords"]),
             "batch_size": case["batch_size"]}
    return vfe, sc, batch
