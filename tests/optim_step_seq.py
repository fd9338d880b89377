"""The contract of the optimiser step (csrc/optim_step.hip) restated in numpy, float32 operation by float32
operation and chunk partial by chunk partial, plus the exact (float64) value of a step and the first-order float32 bound around
it.  Everything the GPU tests compare bit for bit comes from here; nothing here imports the library."""
import numpy as np

F = np.float32
CH = 4096
BLOCK = 256
U = 2.0 ** -24                      # unit roundoff of float32
TINY = 2.0 ** -149


def block_sum(acc):
    """256 float64 lane sums -> one: a[l] += a[l + s] for s = 32 .. 1 inside each wavefront of 64, then ((w0 + w1) + w2) + w3"""
    a = np.array(acc, dtype=np.float64).reshape(4, 64)
    s = 32
    while s >= 1:
        a[:, :s] = a[:, :s] + a[:, s:2 * s]
        s //= 2
    return ((a[0, 0] + a[1, 0]) + a[2, 0]) + a[3, 0]


def chunk_partials(g):
    """the float64 partial of every chunk of one gradient: lane l of pass j owns elements 1024 j + 4 l .. + 3, summed in that order"""
    g = np.asarray(g, dtype=F).reshape(-1)
    out = []
    with np.errstate(all="ignore"):
        for c in range(-(-g.size // CH)):
            x = np.zeros(CH, dtype=np.float64)
            part = g[c * CH:(c + 1) * CH].astype(np.float64)
            x[:part.size] = part
            sq = (x * x).reshape(CH // (4 * BLOCK), BLOCK, 4)          # pass, lane, element
            acc = np.zeros(BLOCK, dtype=np.float64)
            for j in range(sq.shape[0]):
                for q in range(4):
                    acc = acc + sq[j, :, q]
            out.append(block_sum(acc))
    return out


def resum(partials):
    """lane l adds partials l, l + 256, ... in that order, then block_sum"""
    acc = np.zeros(BLOCK, dtype=np.float64)
    p = np.asarray(partials, dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(0, p.size, BLOCK):
            row = p[i:i + BLOCK]
            acc[:row.size] = acc[:row.size] + row
        return block_sum(acc)


def total_norm(grads):
    """(float) sqrt of the float64 sum over the gradients (None and empty ones own no chunk), in the order given"""
    partials = []
    for g in grads:
        if g is not None:
            partials += chunk_partials(g)
    with np.errstate(all="ignore"):
        return F(np.sqrt(np.float64(resum(partials))))


def clip_coef(norm, max_norm):
    with np.errstate(all="ignore"):
        c = (F(1) / (F(norm) + F(1e-6))) * F(max_norm)
    return F(1) if c > F(1) else c          # a NaN stays a NaN


def clip(g, coef):
    with np.errstate(all="ignore"):
        return np.asarray(g, dtype=F) * F(coef)


def host_scalars(lr, beta1, beta2, eps, t, dec=1.0):
    """Python doubles, rounded to float32 once; omw = fl(1 - w) in float32"""
    w = F(1 - beta1)
    return dict(dec=F(dec), w=w, omw=F(1) - w, b2=F(beta2), omb2=F(1 - beta2), bc2s=F((1 - beta2 ** t) ** 0.5), eps=F(eps),
                nss=F(-(lr / (1 - beta1 ** t))), high=bool(w >= F(0.5)))


def adam(p, m, v, g, s):
    """one tensor's step in float32 -> p, m, v"""
    p, m, v, g = (np.asarray(a, dtype=F) for a in (p, m, v, g))
    with np.errstate(all="ignore"):
        p1 = p * s["dec"]
        d = g - m
        m = g - d * s["omw"] if s["high"] else m + s["w"] * d
        v = (v * s["b2"]) + (s["omb2"] * (g * g))
        den = np.sqrt(v) / s["bc2s"] + s["eps"]
        return p1 + s["nss"] * (m / den), m, v


def decay(p, dec):
    with np.errstate(all="ignore"):
        return np.asarray(p, dtype=F) * F(dec)


def exact(p, m, v, g, lr, beta1, beta2, eps, t, dec, variant=None, wd=0.0):
    """the step in float64 with the scalars in Python doubles -> p, m, v.  variant: one of the deliberately wrong steps --
    'l2' the decay folded into the gradient, 'decay_after' the decay applied to the updated parameter"""
    p, m, v, g = (np.asarray(a, dtype=np.float64) for a in (p, m, v, g))
    with np.errstate(all="ignore"):
        if variant == "l2":
            g = g + wd * p
            dec = 1.0
        m = m + (1 - beta1) * (g - m)
        v = v * beta2 + (1 - beta2) * g * g
        den = np.sqrt(v) / (1 - beta2 ** t) ** 0.5 + eps
        upd = -(lr / (1 - beta1 ** t)) * (m / den)
        return ((p + upd) * dec if variant == "decay_after" else p * dec + upd), m, v


def bound(p, m, v, g, lr, beta1, beta2, eps, t, dec):
    """First-order float32 error bounds of p, m, v after a step around exact() (derived in DESIGN.md section 7w): every rounded
    scalar and every float32 operation contributes one unit roundoff U of its result; the division by bc2s counts three (the
    scalar, and a reciprocal-then-multiply form of the division).  Needs beta1 > 0.5 (the first lerp branch)."""
    assert 1 - beta1 < 0.5
    p, m, v, g = (np.asarray(a, dtype=np.float64) for a in (p, m, v, g))
    P, M, V = exact(p, m, v, g, lr, beta1, beta2, eps, t, dec)
    with np.errstate(all="ignore"):
        em = U * (3 * np.abs((1 - beta1) * (g - m)) + np.abs(M))
        ev = U * (2 * v * beta2 + 3 * (1 - beta2) * g * g + V)
        root = np.sqrt(V)
        bc = (1 - beta2 ** t) ** 0.5
        q = root / bc
        eroot = np.where(V > 0, ev / (2 * np.where(V > 0, root, 1.0)), 0.0) + U * root
        den = q + eps
        eden = eroot / bc + 3 * U * q + U * eps + U * den
        r = M / den
        er = em / den + np.abs(r) * eden / den + U * np.abs(r)
        upd = (lr / (1 - beta1 ** t)) * np.abs(r)
        eupd = (lr / (1 - beta1 ** t)) * er + 2 * U * upd
        ep = 2 * U * np.abs(p * dec) + eupd + U * np.abs(P)
    slack = 1.001                      # the second-order terms and the float64 arithmetic of this function
    return ep * slack + TINY, em * slack + TINY, ev * slack + TINY


def step_tensors(tensors, max_norm=None, fused_order=None):
    """One step over `tensors`: dicts with p, g (None: no gradient), m, v (None before the first gradient), t (steps so far),
    lr, beta1, beta2, eps, dec (1.0: not decayed), frozen.  With max_norm the gradients are clipped first (all of them,
    in the tensors' order).  -> (new tensors, total_norm or None, clipped gradients)"""
    norm = coef = None
    grads = [x["g"] for x in tensors]
    if max_norm is not None:
        norm = total_norm([g for g in grads if g is not None and np.size(g)])
        coef = clip_coef(norm, max_norm)
        grads = [None if g is None else clip(g, coef) for g in grads]
    out = []
    for x, g in zip(tensors, grads):
        y = dict(x)
        if x.get("frozen") and g is None:
            out.append(y)
            continue
        if g is None:
            y["p"] = decay(x["p"], x["dec"])
        else:
            t = x["t"] + 1
            m = np.zeros_like(x["p"]) if x["m"] is None else x["m"]
            v = np.zeros_like(x["p"]) if x["v"] is None else x["v"]
            y["p"], y["m"], y["v"] = adam(x["p"], m, v, g, host_scalars(x["lr"], x["beta1"], x["beta2"], x["eps"], t, x["dec"]))
            y["t"] = t
        out.append(y)
    return out, norm, grads


def _differ(a, b):
    """elementwise: other bits, except that a NaN equals a NaN (the sign and payload of a generated NaN are the processor's)"""
    return (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and not _differ(a, b).any()


def first_difference(a, b):
    a, b = np.ascontiguousarray(a, dtype=F).reshape(-1), np.ascontiguousarray(b, dtype=F).reshape(-1)
    if a.shape != b.shape:
        return f"shapes {a.shape} and {b.shape}"
    bad = np.flatnonzero(_differ(a, b))
    return "equal" if not bad.size else f"{bad.size} of {a.size} elements differ, first at {bad[0]}: {a[bad[0]]!r} against {b[bad[0]]!r}"
