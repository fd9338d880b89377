"""GPU: the optimiser-step kernels (csrc/optim_step.hip) through the drop-ins of
modest_amd.utils.optim_step -- clip_grad_norm_, step and clip_and_step on a stand-in for the reference's OptimWrapper -- against
the numpy restatement tests/optim_step_seq.py BIT FOR BIT (a NaN equals a NaN): parameters, exp_avg, exp_avg_sq, step counts,
total_norm and the clipped gradients; the recorded scenes (tests/golden/optim_step.npz) also within the derived bound of the
exact step.  A mismatch reports the element.

One documented difference from torch: total_norm is (float) sqrt of a float64 sum, so gradients of 1e25 give a finite norm where
torch's float32 sum overflows to inf (test_values_gradients_of_1e25)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import optim_step_seq as seq
from optim_step_cases import CH, SIZES, Wrapper, make_wrapper, onecycle, scenes, shape_sets, values
from modest_amd.utils import optim_step as osd

pytestmark = pytest.mark.gpu
F = np.float32
WD, BETA2, EPS = 0.01, 0.99, 1e-8


def initial(sizes, seed=0, bn=(), frozen=()):
    return [dict(p=values(n, seed + 7 * i), m=None, v=None, t=0.0, bn=i in bn, frozen=i in frozen) for i, n in enumerate(sizes)]


def schedule(tensors, n_steps, seed=100, none=(), scale=1.0, first=0):
    """n_steps of (lr, mom, gradients); none: (step, tensor) pairs without a gradient; a frozen tensor never has one"""
    steps = []
    for k in range(n_steps):
        lr, mom = onecycle(first + k)
        grads = [None if (k, i) in none or x["frozen"] else values(x["p"].size, seed + 1000 * k + i, scale) for i, x in enumerate(tensors)]
        steps.append(dict(lr=lr, mom=mom, grads=grads))
    return steps


def order_of(tensors):
    return [i for i, x in enumerate(tensors) if not x["bn"]] + [i for i, x in enumerate(tensors) if x["bn"]]


def restate(tensors, steps, max_norm=None, bn_wd=True):
    """-> (tensors after, [norm per step], gradients after the last step: clipped with max_norm) in the groups' order"""
    cur = [dict(tensors[i], beta2=BETA2, eps=EPS) for i in order_of(tensors)]
    norms, grads = [], None
    for st in steps:
        for x, i in zip(cur, order_of(tensors)):
            decays = not x["frozen"] and (not x["bn"] or bn_wd)
            x.update(lr=st["lr"], beta1=st["mom"], g=st["grads"][i], dec=1 - WD * st["lr"] if decays else 1.0)
        cur, norm, grads = seq.step_tensors(cur, max_norm)
        norms.append(norm)
    return cur, norms, grads


def carved(a, off, gpu):
    """a device copy of `a` that starts `off` floats behind a 16-byte boundary"""
    flat = torch.zeros(a.size + 8, dtype=torch.float32, device=gpu)
    assert flat.data_ptr() % 16 == 0
    t = flat[off:off + a.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return t


def on_device(tensors, steps, gpu, mode, max_norm=None, carve=(0, 0, 0), bn_wd=True, wrapper=None, keep=None, no_sync=False):
    """the same through the drop-ins; mode: 'step', 'pair' (clip_grad_norm_ then step) or 'fused' (clip_and_step).  Nothing is
    read back before the last step is enqueued."""
    order = order_of(tensors)
    params = [torch.nn.Parameter(carved(tensors[i]["p"], carve[0], gpu), requires_grad=not tensors[i]["frozen"]) for i in order]
    w = wrapper or make_wrapper([p for p, i in zip(params, order) if not tensors[i]["bn"]],
                                [p for p, i in zip(params, order) if tensors[i]["bn"]], wd=WD, betas=(0.9, BETA2))
    w.bn_wd = bn_wd
    for p, i in zip(params, order):
        x = tensors[i]
        if x["m"] is not None or (any(carve) and not x["frozen"]):
            zero = np.zeros_like(x["p"])
            w.opt.state[p] = dict(step=torch.tensor(float(x["t"]), dtype=torch.float32),
                                  exp_avg=carved(zero if x["m"] is None else x["m"], carve[2], gpu),
                                  exp_avg_sq=carved(zero if x["v"] is None else x["v"], carve[2], gpu))
    norms = []
    staged = [[None if st["grads"][i] is None else carved(st["grads"][i], carve[1], gpu) for i in order] for st in steps]
    if no_sync:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")        # a synchronising call of torch's between here and the last step raises
    try:
        for st, grads in zip(steps, staged):
            w.hyper(st["lr"], st["mom"])
            for p, g in zip(params, grads):
                p.grad = g
            if mode == "pair":
                norms.append(osd.clip_grad_norm_(iter(params), max_norm))
                osd.step(w)
            elif mode == "fused":
                norms.append(osd.clip_and_step(w, max_norm))
            else:
                osd.step(w)
    finally:
        if no_sync:
            torch.cuda.set_sync_debug_mode("default")
    if keep is not None:
        keep.update(w=w, params=params)
    out = []
    for p in params:
        st = w.opt.state.get(p, {})
        out.append(dict(p=p.detach().cpu().numpy(), m=st["exp_avg"].cpu().numpy() if st else None,
                        v=st["exp_avg_sq"].cpu().numpy() if st else None, t=float(st["step"]) if st else 0.0))
    return out, [None if n is None else n.cpu().numpy() for n in norms], [None if p.grad is None else p.grad.cpu().numpy() for p in params]


def assert_same(got, want, what=""):
    (gt, gn, gg), (wt, wn, wg) = got, want
    assert len(gt) == len(wt)
    for i, (a, b) in enumerate(zip(gt, wt)):
        assert a["t"] == b["t"], f"{what} tensor {i}: step count {a['t']} against {b['t']}"
        for key in "pmv":
            assert (a[key] is None) == (b[key] is None), f"{what} tensor {i} {key}: state on one side only"
            if a[key] is not None:
                assert seq.same_bits(a[key], b[key]), f"{what} tensor {i} {key}: {seq.first_difference(a[key], b[key])}"
    for k, (a, b) in enumerate(zip(gn, wn)):
        if b is not None:
            assert a.shape == () and a.dtype == np.float32 and seq.same_bits(a, b), f"{what} total_norm of step {k}: {a!r} against {b!r}"
    if wg is not None:
        for i, (a, b) in enumerate(zip(gg, wg)):
            assert (a is None) == (b is None) and (a is None or seq.same_bits(a, b)), f"{what} gradient {i}: {a is None or seq.first_difference(a, b)}"


def check(tensors, steps, gpu, mode="pair", max_norm=10.0, **kw):
    want = restate(tensors, steps, max_norm if mode != "step" else None, kw.get("bn_wd", True))
    got = on_device(tensors, steps, gpu, mode, max_norm, **kw)
    assert_same(got, want if mode != "fused" else (want[0], want[1], None), mode)
    return got, want


def test_chunk_is_what_the_restatement_assumes(gpu):
    from modest_amd import ops
    assert ops.optim_chunk() == CH == seq.CH and ops.optim_workspace_bytes(3, 5) >= 3 * 88 + 5 * 8 + 8
    assert ops.OPTIM_STATIC.itemsize == 40 and ops.OPTIM_STEP.itemsize == 48


def test_sizes(gpu):
    tensors = initial(SIZES, bn=(3, 7))
    check(tensors, schedule(tensors, 2, scale=3.0), gpu)             # clips
    check(tensors, schedule(tensors, 2, scale=0.01), gpu)            # does not
    check(tensors, schedule(tensors, 2), gpu, mode="step")


@pytest.mark.parametrize("carve", [(1, 2, 3), (2, 3, 1), (3, 1, 2), (0, 0, 1), (0, 1, 0), (1, 0, 0)])
def test_alignment(gpu, carve):
    tensors = initial(SIZES, bn=(3, 7))
    steps = schedule(tensors, 2, scale=3.0)
    aligned = on_device(tensors, steps, gpu, "pair", 10.0, carve=(0, 0, 0))
    got, _ = check(tensors, steps, gpu, carve=carve)
    assert_same(got, aligned, "against the aligned run")
    assert_same(on_device(tensors, steps, gpu, "fused", 10.0, carve=carve), (aligned[0], aligned[1], None), "fused against the aligned run")


def test_gradients_none(gpu):
    tensors = initial((300, 5000, 64, 17, 40), bn=(3,), frozen=(4,))
    # step 0: tensor 0 has no gradient -> only the decay, no state; step 1 of 3: tensor 1 has none -> its count falls behind
    steps = schedule(tensors, 3, none=((0, 0), (1, 1)))
    first = check(tensors, steps[:1], gpu)[0][0]
    assert first[0]["m"] is None and first[0]["t"] == 0.0
    assert seq.same_bits(first[0]["p"], seq.decay(tensors[0]["p"], 1 - WD * steps[0]["lr"])) and not seq.same_bits(first[0]["p"], tensors[0]["p"])
    got, _ = check(tensors, steps, gpu)
    assert [x["t"] for x in got[0]] == [2.0, 2.0, 3.0, 0.0, 3.0]      # others 0, 1, 2, 4 (frozen), then the BN tensor
    frozen = got[0][3]
    assert frozen["m"] is None and seq.same_bits(frozen["p"], tensors[4]["p"])      # neither decay nor update
    check(tensors, steps, gpu, mode="fused")
    check(tensors, steps, gpu, bn_wd=False)                            # the BN group is not decayed


def test_many_tensors(gpu):
    rs = np.random.RandomState(5)
    tensors = initial([int(n) for n in rs.randint(1, 131, size=700)], bn=set(range(600, 700)))
    check(tensors, schedule(tensors, 1, scale=2.0), gpu)
    check(tensors, schedule(tensors, 1, scale=2.0), gpu, mode="fused")


def test_schedule_of_eight_steps_enqueued_back_to_back(gpu):
    tensors = initial((CH + 3, 700, 64, 31), bn=(2,))
    steps = schedule(tensors, 8, scale=0.5)
    assert len({(s["lr"], s["mom"]) for s in steps}) == 8
    got = on_device(tensors, steps, gpu, "pair", 10.0, no_sync=True)
    assert_same(got, restate(tensors, steps, 10.0), "eight steps")
    check(tensors, steps + schedule(tensors, 4, seed=900, first=8), gpu, mode="fused")      # past a whole ring of slots


def one(n, g, seed=1):
    tensors = initial((n,), seed=seed)
    return tensors, [dict(lr=1e-3, mom=0.9, grads=[np.asarray(g, dtype=F)])]


def test_values_zero_gradients_and_the_norm_around_max_norm(gpu):
    tensors, steps = one(1000, np.zeros(1000))
    got, _ = check(tensors, steps, gpu)
    assert float(got[1][0]) == 0.0
    g = np.zeros(CH + 5, dtype=F)
    for last, side in ((F(7.99999), "under"), (F(8.00001), "over")):      # 6 and 8 give a norm of 10: eight millionths either side
        g[0], g[CH + 2] = F(6.0), last
        tensors, steps = one(CH + 5, g.copy())
        got, want = check(tensors, steps, gpu)
        coef = seq.clip_coef(want[1][0], 10.0)
        assert abs(float(want[1][0]) - 10) < 1e-5 and ((coef == 1) if side == "under" else (coef < 1)), (side, want[1][0], coef)
        assert seq.same_bits(got[2][0], g) == (side == "under")
        check(tensors, steps, gpu, mode="fused")
    tensors, steps = one(64, values(64, 3) * F(1e-3))                  # far under: coef is 1 and the gradients keep their bits
    got, want = check(tensors, steps, gpu)
    assert seq.same_bits(got[2][0], steps[0]["grads"][0])


def test_values_beta1_of_0_3_takes_the_other_lerp_branch(gpu):
    tensors = initial((CH + 9, 77), bn=(1,))
    steps = [dict(s, mom=0.3) for s in schedule(tensors, 2)]
    assert seq.host_scalars(1e-3, 0.3, BETA2, EPS, 1.0)["high"]
    got, _ = check(tensors, steps, gpu)
    other = restate(tensors, [dict(s, mom=0.6) for s in steps], 10.0)
    assert not seq.same_bits(got[0][0]["m"], other[0][0]["m"])
    check(tensors, steps, gpu, mode="fused")


@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_values_one_non_finite_element(gpu, poison):
    tensors = initial((500, CH + 1))
    steps = schedule(tensors, 2)
    steps[1]["grads"][1][CH] = poison
    got, _ = check(tensors, steps, gpu)
    nans = sum(int(np.isnan(x["p"]).sum()) for x in got[0])
    assert nans == (500 + CH + 1 if np.isnan(poison) else 1)            # a NaN norm poisons everything, an inf norm gives coef 0
    check(tensors, steps, gpu, mode="fused")


def test_values_gradients_of_1e25(gpu):
    """THE DOCUMENTED DIFFERENCE: our norm stays finite where torch's float32 sum of squares overflows"""
    g = np.full(300, 1e25, dtype=F)
    tensors, steps = one(300, g)
    got, want = check(tensors, steps, gpu)
    assert np.isfinite(got[1][0]) and abs(float(got[1][0]) / (1e25 * np.sqrt(300.0)) - 1) < 1e-6
    p = torch.nn.Parameter(torch.zeros(300, device=gpu))
    p.grad = torch.from_numpy(g).to(gpu)
    assert torch.isinf(torch.nn.utils.clip_grad_norm_([p], 10.0))


def test_state_load_state_dict_clear_and_a_step_of_torchs_own(gpu):
    tensors = initial((CH + 3, 200, 32), bn=(2,))
    steps = schedule(tensors, 4)
    keep = {}
    on_device(tensors, steps[:1], gpu, "pair", 10.0, keep=keep)
    w, params = keep["w"], keep["params"]
    old = [w.opt.state[p]["exp_avg"] for p in params]
    old_bits = [t.clone() for t in old]
    w.load_state_dict(copy.deepcopy(w.state_dict()))                    # as from a checkpoint: every state tensor is another one
    assert all(w.opt.state[p]["exp_avg"] is not o for p, o in zip(params, old))

    def run(k, mode):
        w.hyper(steps[k]["lr"], steps[k]["mom"])
        for p, g in zip(params, steps[k]["grads"]):
            p.grad = torch.from_numpy(g).to(gpu)
        return osd.clip_grad_norm_(params, 10.0), (osd.step(w) if mode == "ours" else Wrapper.step(w))

    def now():
        return [dict(p=p.detach().cpu().numpy(), m=w.opt.state[p]["exp_avg"].cpu().numpy(), v=w.opt.state[p]["exp_avg_sq"].cpu().numpy(),
                     t=float(w.opt.state[p]["step"])) for p in params]
    run(1, "ours")
    want = restate(tensors, steps[:2], 10.0)
    assert_same((now(), [], None), (want[0], [], None), "after load_state_dict")
    assert all(torch.equal(o, b) for o, b in zip(old, old_bits))        # the replaced tensors are no longer written
    run(2, "torch")                                                     # torch's own step runs from the state we left
    want3 = restate(tensors, steps[:3], 10.0)[0]
    for a, b in zip(now(), want3):
        assert a["t"] == b["t"] == 3.0
        for key in "pmv":
            assert np.allclose(a[key], b[key], rtol=1e-4, atol=1e-7), key
    w.clear()                                                           # ... and clear() starts the counts again
    assert all(len(w.opt.state.get(p, {})) == 0 for p in params)
    start = [dict(x, p=a["p"], m=None, v=None, t=0.0) for x, a in zip([tensors[i] for i in order_of(tensors)], now_p(params))]
    run(3, "ours")
    want = restate(start, [dict(steps[3], grads=[steps[3]["grads"][i] for i in order_of(tensors)])], 10.0)
    assert_same((now(), [], None), (want[0], [], None), "after clear()")


def now_p(params):
    return [dict(p=p.detach().cpu().numpy()) for p in params]


def test_fused_path_equals_the_pair_and_leaves_the_gradients(gpu):
    tensors = initial((3 * CH + 11, 900, 64, 5), bn=(2,))
    steps = schedule(tensors, 3, scale=2.0)
    pair = on_device(tensors, steps, gpu, "pair", 10.0)
    fused = on_device(tensors, steps, gpu, "fused", 10.0)
    assert_same(fused, (pair[0], pair[1], None), "fused against the pair")
    order = order_of(tensors)
    for a, b, i in zip(fused[2], pair[2], order):
        assert seq.same_bits(a, steps[-1]["grads"][i]) and not seq.same_bits(b, steps[-1]["grads"][i])      # .grad unscaled / scaled


def test_golden_scenes_on_the_device(gpu):
    for name, recorded in scenes().items():
        for k, st in enumerate(recorded):
            by = {x["name"]: x for x in st["tensors"]}
            tensors = [dict(p=x["p"].reshape(-1), m=None if x["m"] is None else x["m"].reshape(-1),
                            v=None if x["v"] is None else x["v"].reshape(-1), t=x["t"], bn=x["bn"], frozen=x["frozen"]) for x in st["tensors"]]
            assert order_of(tensors) == list(range(len(tensors)))
            x0 = st["tensors"][0]
            raw = [dict(lr=x0["lr"], mom=x0["beta1"], grads=[None if x["g"] is None else x["g"].reshape(-1) for x in st["tensors"]])]
            check(tensors, raw, gpu, max_norm=st["max_norm"])                           # equal to the restatement from the raw gradients
            clipped = [dict(raw[0], grads=[None if x["gc"] is None else x["gc"].reshape(-1) for x in st["tensors"]])]
            got, _ = check(tensors, clipped, gpu, mode="step")                           # ... and from the recorded clipped ones
            for x, y in zip(st["tensors"], got[0]):                                      # within the bound of the exact step
                if x["gc"] is None:
                    continue
                m0 = np.zeros_like(x["p"]) if x["m"] is None else x["m"]
                v0 = np.zeros_like(x["p"]) if x["v"] is None else x["v"]
                args = (x["p"], m0, v0, x["gc"], x["lr"], x["beta1"], x["beta2"], x["eps"], x["t"] + 1, x["dec"])
                for key, e, b in zip("pmv", seq.exact(*args), seq.bound(*args)):
                    e, b, a = e.reshape(-1), b.reshape(-1), y[key].astype(np.float64)
                    fin = np.isfinite(e)
                    assert np.array_equal(np.isnan(a), np.isnan(e)) and np.all(np.abs(a - e)[fin] <= b[fin]), (name, k, x["name"], key)


def test_determinism_on_the_pointpillars_set(gpu):
    rows = shape_sets()["pointpillars_lyft"]
    sizes = [int(np.prod(r["shape"])) for r in rows]
    assert 4_700_000 < sum(sizes) < 4_900_000
    tensors = initial(sizes, bn={i for i, r in enumerate(rows) if r["bn"]})
    steps = schedule(tensors, 1, scale=0.05)
    a = on_device(tensors, steps, gpu, "pair", 10.0)
    b = on_device(tensors, steps, gpu, "pair", 10.0)
    assert_same(a, b, "second run")
    assert_same(on_device(tensors, steps, gpu, "fused", 10.0), (a[0], a[1], None), "fused")
    assert_same(a, restate(tensors, steps, 10.0), "restatement")


def device_events(fn):
    """kernel launches and device copies that fn() causes, from torch's profiler"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))


def raises(exc, match, fn):
    with pytest.raises(exc, match=match):
        fn()


def test_grad_norm_op_alone(gpu):
    """ops.optim_grad_norm (the norm kernel and the one-workgroup finishing launch): gradients present and absent, several chunks,
    views 1, 2 and 3 floats off a 16-byte boundary"""
    from modest_amd import ops
    sizes, offs, absent = [5, CH + 1, 3 * CH + 7, 64, 1, 2 * CH], [0, 1, 2, 3, 0, 3], {3}
    host = [values(n, 40 + i, 2.0) for i, n in enumerate(sizes)]
    grads = [None if i in absent else carved(g, o, gpu) for i, (g, o) in enumerate(zip(host, offs))]
    tab = osd._Tables()
    zeros = [0] * len(sizes)
    static = tab.build(gpu, zeros, zeros, zeros, sizes)
    step = tab.step_table([0 if g is None else g.data_ptr() for g in grads])
    assert list(step["norm_first"]) == [0, 1, 3, -1, 7, 8]
    norm = torch.full((), -1.0, dtype=torch.float32, device=gpu)
    assert ops.optim_grad_norm(static, step, tab.workspace, norm) is norm
    want = seq.total_norm([g for i, g in enumerate(host) if i not in absent])
    assert seq.same_bits(norm.cpu().numpy(), want), (norm.item(), want)
    for g, h in zip(grads, host):
        assert g is None or seq.same_bits(g.cpu().numpy(), h)                  # the norm alone writes no gradient
    step = tab.step_table([0] * len(sizes))                                     # no gradient at all: a norm of 0
    ops.optim_grad_norm(static, step, tab.workspace, norm, upload_static=False)
    assert float(norm) == 0.0


def test_finish_launch_gives_the_same_bits(gpu, monkeypatch):
    tensors = initial((3 * CH + 11, 900, 64, 5, CH), bn=(2,))
    steps = schedule(tensors, 2, scale=2.0, none=((1, 1),))
    want = restate(tensors, steps, 10.0)
    monkeypatch.setattr(osd, "FINISH_LAUNCH", True)
    assert_same(on_device(tensors, steps, gpu, "pair", 10.0, carve=(1, 2, 3)), want, "pair with a finishing launch")
    assert_same(on_device(tensors, steps, gpu, "fused", 10.0), (want[0], want[1], None), "fused with a finishing launch")


def test_a_call_the_library_refuses_leaves_the_optimiser_as_it_was(gpu, monkeypatch):
    from modest_amd import ops
    tensors = initial((CH + 3, 200), bn=(1,))
    steps = schedule(tensors, 2)
    keep = {}
    on_device(tensors, steps[:1], gpu, "step", keep=keep)
    w, params = keep["w"], keep["params"]
    fresh = torch.nn.Parameter(torch.ones(7, device=gpu))                       # a tensor that gets its state in the failing call
    w.opt.param_groups[0]["params"].append(fresh)
    for p, g in zip(params + [fresh], steps[1]["grads"] + [np.ones(7, dtype=F)]):
        p.grad = torch.from_numpy(g).to(gpu)
    w.opt.param_groups[0]["weight_decay"] = 0.5
    before = [p.detach().clone() for p in params]

    def refuse(*a, **k):
        raise ops._lib.ModestHipError("refused")
    monkeypatch.setattr(ops, "optim_step", refuse)
    with pytest.raises(ops._lib.ModestHipError):
        osd.step(w)
    assert [float(w.opt.state[p]["step"]) for p in params] == [1.0, 1.0] and len(w.opt.state.get(fresh, {})) == 0
    assert w.opt.param_groups[0]["weight_decay"] == 0.5 and all(torch.equal(a, p) for a, p in zip(before, params))
    monkeypatch.undo()
    osd.step(w)
    assert [float(w.opt.state[p]["step"]) for p in params + [fresh]] == [2.0, 2.0, 1.0]


def test_refusals_launch_nothing(gpu):
    from modest_amd import ops
    lin = torch.nn.Linear(8, 4).to(gpu)
    for p in lin.parameters():
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in lin.parameters()]
    half = torch.nn.Linear(8, 4).to(gpu).half()
    t = torch.nn.Parameter(torch.zeros(4, 6, device=gpu).t())
    t.grad = torch.ones(6, 4, device=gpu)
    w = make_wrapper([t] + list(lin.parameters()), [])
    host = torch.nn.Linear(8, 4)
    for p in host.parameters():
        p.grad = torch.ones_like(p)
    assert device_events(lambda: osd.step(make_wrapper(lin.parameters(), []))) > 0      # the counter sees a step that runs
    for p, b in zip(lin.parameters(), before):
        p.data.copy_(b)
    not32 = "parameters that are not contiguous float32"
    refused = [
        lambda: raises(NotImplementedError, "amsgrad", lambda: osd.step(make_wrapper(lin.parameters(), [], amsgrad=True))),
        lambda: raises(NotImplementedError, not32, lambda: osd.step(make_wrapper(half.parameters(), []))),
        lambda: raises(NotImplementedError, not32, lambda: osd.step(w)),
        lambda: raises(NotImplementedError, not32, lambda: osd.clip_and_step(w, 10.0)),
        lambda: raises(ValueError, "more than one device", lambda: osd.step(make_wrapper(list(host.parameters()) + list(lin.parameters()), []))),
    ]
    # ... and those of the ops themselves: a table of another dtype, a short workspace, an output on the host or of another type
    tab = osd._Tables()
    static = tab.build(gpu, [0], [0], [0], [32])
    step = tab.step_table([lin.weight.grad.data_ptr()])
    norm = torch.zeros((), dtype=torch.float32, device=gpu)
    on_host, as_double, two = norm.cpu(), norm.double(), torch.zeros(2, device=gpu)      # made here: making them launches
    refused += [
        lambda: raises(TypeError, "ops.OPTIM_STATIC", lambda: ops.optim_clip(static.view(np.uint8), step, 10.0, tab.workspace, norm)),
        lambda: raises(TypeError, "ops.OPTIM_STEP", lambda: ops.optim_clip(static, step[:0], 10.0, tab.workspace, norm)),
        lambda: raises(ValueError, "the table holds no tensor", lambda: ops.optim_grad_norm(static[:0], step[:0], tab.workspace, norm)),
        lambda: raises(ValueError, "bytes, .* are needed", lambda: ops.optim_clip(static, step, 10.0, tab.workspace[:256], norm)),
        lambda: raises(ValueError, "norm_out must be a device tensor", lambda: ops.optim_clip(static, step, 10.0, tab.workspace, on_host)),
        lambda: raises(TypeError, "norm_out must be torch.float32", lambda: ops.optim_norm_step(static, step, 10.0, tab.workspace, as_double)),
        lambda: raises(ValueError, "norm_out must be one float32", lambda: ops.optim_grad_norm(static, step, tab.workspace, two)),
        lambda: raises(ops._lib.ModestHipError, "parameter pointer", lambda: ops.optim_step(static, step, tab.workspace)),
    ]
    for k, fn in enumerate(refused):
        assert device_events(fn) == 0, f"refusal {k} launched something"
    assert len(w.opt.state) == 0 and all(torch.equal(a, p) for a, p in zip(before, lin.parameters()))
    assert torch.equal(lin.weight.grad, torch.ones_like(lin.weight))


def test_hand_overs_to_torchs_own_function(gpu):
    lin = torch.nn.Linear(8, 4).to(gpu)
    for p in lin.parameters():
        p.grad = torch.ones_like(p)
    host = torch.nn.Linear(8, 4)
    for p in host.parameters():
        p.grad = torch.ones_like(p)
    assert osd.clip_grad_norm_(host.parameters(), 1.0).device.type == "cpu"             # host tensors: torch's function
    n1 = osd.clip_grad_norm_(lin.parameters(), 100.0, norm_type=1)                     # norm_type 1: torch's function
    assert float(n1) == 36.0
    g16 = torch.nn.Parameter(torch.zeros(4, device=gpu, dtype=torch.float16))
    g16.grad = torch.ones_like(g16)
    assert osd.clip_grad_norm_([g16], 100.0).dtype == torch.float16                    # not float32: torch's function


def test_resources_no_scratch():
    from modest_amd import build as mb
    res = json.load(open(os.path.join(mb.LIBDIR, "kernel_resources.json")))
    ours = {k: v for k, v in res.items() if v["file"] == "optim_step.hip"}
    assert len(ours) == 7      # the norm, its finishing launch, the clip (2 ways to the coefficient), the step (3)
    for k, v in ours.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, k
