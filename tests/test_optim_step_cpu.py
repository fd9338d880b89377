"""CPU: the contract of the optimiser step as tests/optim_step_seq.py restates it, against the reference's
own build_optimizer / OneCycle / clip_grad_norm_ run recorded in tests/golden/optim_step.npz by tools/make_golden_optim_step.py:
(a) the clipped gradients bit for bit from the recorded norm, (b) both norms within their derived bounds of the float64 sum,
(c) p, m, v of the recording and of the restatement within the first-order float32 bound of the exact step, (d) equal NaN / inf
patterns and step counts, (e) four deliberately wrong steps leave the bound; then the host scalars of a OneCycle schedule and
the state format of the drop-in's host part."""
import math

import numpy as np
import pytest
import torch

import optim_step_seq as seq
from optim_step_cases import CH, make_wrapper, onecycle, scenes
from modest_amd.utils import optim_step as osd

F = np.float32


@pytest.fixture(scope="module")
def gold():
    return scenes()


def all_steps(gold):
    for name, steps in gold.items():
        for k, st in enumerate(steps):
            yield f"{name} step {k}", st


def test_a_clipped_gradients_from_the_recorded_norm_bit_for_bit(gold):
    seen = set()
    for where, st in all_steps(gold):
        coef = seq.clip_coef(st["norm"], st["max_norm"])
        seen.add("nan" if np.isnan(coef) else "clips" if coef < 1 else "keeps")
        for x in st["tensors"]:
            if x["g"] is not None:
                assert seq.same_bits(seq.clip(x["g"], coef), x["gc"]), f"{where} {x['name']}: {seq.first_difference(seq.clip(x['g'], coef), x['gc'])}"
    assert seen == {"nan", "clips", "keeps"}
    # the other form of the coefficient, max_norm / (total_norm + 1e-6), is NOT what torch evaluates
    other = 0
    for where, st in all_steps(gold):
        with np.errstate(all="ignore"):
            c = F(st["max_norm"]) / (F(st["norm"]) + F(1e-6))
        c = F(1) if c > 1 else c
        other += sum(not seq.same_bits(seq.clip(x["g"], c), x["gc"]) for x in st["tensors"] if x["g"] is not None)
    assert other > 0


def test_b_both_norms_within_their_bounds_of_the_float64_sum(gold):
    chunks = 0
    for where, st in all_steps(gold):
        by_name = {x["name"]: x["g"] for x in st["tensors"]}
        grads = [by_name[n] for n in st["model_order"] if by_name[n] is not None]
        ours, theirs = seq.total_norm(grads), F(st["norm"])
        chunks = max(chunks, max(-(-g.size // CH) for g in grads))
        flat = np.concatenate([g.reshape(-1) for g in grads]).astype(np.float64)
        if not np.isfinite(flat).all():
            assert (np.isnan(ours) and np.isnan(theirs)) or (ours == theirs == F(np.inf)), where
            continue
        exact = math.sqrt(math.fsum(flat * flat))
        # ours: a float64 sum of exact squares (relative error <= n 2^-53), one float64 sqrt, one rounding to float32 (<= U)
        assert abs(float(ours) - exact) <= 2 * seq.U * exact, (where, ours, exact)
        # theirs: float32 squares and float32 sums of n terms in some order, the per-tensor norms summed again: (n + 8) U
        assert abs(float(theirs) - exact) <= (flat.size + 8) * seq.U * exact, (where, theirs, exact)
    assert chunks > 1                             # some scene has a tensor of more than one chunk


def test_c_d_steps_within_the_bound_of_the_exact_value_and_equal_patterns(gold):
    worst = {"recording": 0.0, "restatement": 0.0}
    for where, st in all_steps(gold):
        start = [dict(x, g=x["gc"]) for x in st["tensors"]]
        ours, _, _ = seq.step_tensors(start)
        for x, y in zip(st["tensors"], ours):
            tag = f"{where} {x['name']}"
            assert y["t"] == x["t1"], tag                                    # (d) the step counts
            if x["gc"] is None:
                assert x["t1"] == x["t"] and (x["m1"] is None) == (x["m"] is None), tag
                want = x["p"].astype(np.float64) * x["dec"]
                for who, got in (("recording", x["p1"]), ("restatement", y["p"])):
                    assert np.all(np.abs(got - want) <= 2 * seq.U * np.abs(want) + seq.TINY), (tag, who)
                if x["frozen"]:
                    assert seq.same_bits(x["p1"], x["p"]) and seq.same_bits(y["p"], x["p"]), tag
                continue
            m0 = np.zeros_like(x["p"]) if x["m"] is None else x["m"]
            v0 = np.zeros_like(x["p"]) if x["v"] is None else x["v"]
            args = (x["p"], m0, v0, x["gc"], x["lr"], x["beta1"], x["beta2"], x["eps"], x["t"] + 1, x["dec"])
            exact, bounds = seq.exact(*args), seq.bound(*args)
            for who, got in (("recording", (x["p1"], x["m1"], x["v1"])), ("restatement", (y["p"], y["m"], y["v"]))):
                for what, a, e, b in zip("pmv", got, exact, bounds):
                    fin = np.isfinite(e)
                    assert np.array_equal(np.isnan(a), np.isnan(e)) and np.array_equal(np.isinf(a), np.isinf(e)), (tag, who, what)   # (d)
                    err = np.abs(a.astype(np.float64) - e)[fin]
                    assert np.all(err <= b[fin]), (tag, who, what, float(np.max(err / b[fin])))
                    if err.size:
                        worst[who] = max(worst[who], float(np.max(err / b[fin])))
    print("largest error over bound:", worst)
    assert 0 < worst["recording"] <= 1 and 0 < worst["restatement"] <= 1


def test_d_non_finite_gradients_poison_what_torch_poisons(gold):
    nan, inf = gold["nan"][-1], gold["inf"][-1]
    for x in nan["tensors"]:
        if x["gc"] is not None:
            assert np.isnan(x["p1"]).all() and x["p1"].size          # a NaN norm: every gradient, so every parameter
    hit = [x for x in inf["tensors"] if x["gc"] is not None and np.isnan(x["p1"]).any()]
    assert len(hit) == 1 and int(np.isnan(hit[0]["p1"]).sum()) == 1       # an inf norm: coef 0, only inf * 0 is a NaN


@pytest.mark.parametrize("variant", ["l2", "shared_t", "decay_after", "prev_beta1"])
def test_e_a_deliberately_wrong_step_leaves_the_bound(gold, variant):
    outside = 0
    for name, steps in gold.items():
        for k, st in enumerate(steps):
            shared = max(x["t1"] for x in st["tensors"])
            prev = steps[k - 1]["tensors"][0]["beta1"] if k else None
            for x in st["tensors"]:
                if x["gc"] is None or not np.isfinite(x["gc"]).all():
                    continue
                m0 = np.zeros_like(x["p"]) if x["m"] is None else x["m"]
                v0 = np.zeros_like(x["p"]) if x["v"] is None else x["v"]
                right = (x["p"], m0, v0, x["gc"], x["lr"], x["beta1"], x["beta2"], x["eps"], x["t"] + 1, x["dec"])
                kw = {}
                wrong = list(right)
                if variant == "shared_t":
                    wrong[8] = shared
                elif variant == "prev_beta1":
                    if prev is None:
                        continue
                    wrong[5] = prev
                else:
                    kw = dict(variant=variant, wd=x["wd"] if x["dec"] != 1.0 else 0.0)
                got, exact, bounds = seq.exact(*wrong, **kw), seq.exact(*right), seq.bound(*right)
                outside += int(np.sum(np.abs(got[0] - exact[0]) > bounds[0]))
    assert outside > 0, f"the variant {variant} stays within the bound on every scene: the scenes cannot tell it from the contract"


def test_host_scalars_of_a_onecycle_schedule():
    seen_high = False
    for k in range(20):
        lr, mom = onecycle(k)
        for t in (1.0, 2.0, float(k + 1), 1000.0):
            (dec, w, omw, b2, omb2, bc2s, eps, nss), flags = osd.host_scalars(lr, mom, 0.99, 1e-8, t, 1 - 0.01 * lr)
            ref = seq.host_scalars(lr, mom, 0.99, 1e-8, t, 1 - 0.01 * lr)
            got = dict(dec=dec, w=w, omw=omw, b2=b2, omb2=omb2, bc2s=bc2s, eps=eps, nss=nss)
            for key, val in got.items():
                assert type(val) is np.float32 and val.tobytes() == ref[key].tobytes(), (k, t, key)
            assert flags == 0 and not ref["high"]
            assert bc2s == F(math.sqrt(1 - 0.99 ** t)) and nss == F(-lr / (1 - mom ** t)) and dec == F(1 - 0.01 * lr)
    assert abs(onecycle(0)[0] - 0.0003) < 1e-12 and onecycle(0)[1] == 0.95 and abs(onecycle(8)[0] - 0.003) < 1e-12 and abs(onecycle(8)[1] - 0.85) < 1e-12
    for beta1 in (0.5, 0.3):                                       # w >= 0.5: the other branch of lerp
        s, flags = osd.host_scalars(1e-3, beta1, 0.99, 1e-8, 3.0)
        assert flags == 1 and seq.host_scalars(1e-3, beta1, 0.99, 1e-8, 3.0)["high"] and s[2] == F(1) - s[1]
        seen_high = True
    assert seen_high


def test_the_state_our_host_part_leaves_is_torchs_own_format():
    torch.manual_seed(0)
    lin, bn, idle = torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3), torch.nn.Linear(3, 3)
    w = make_wrapper(list(lin.parameters()) + list(idle.parameters()), bn.parameters())
    w.hyper(*onecycle(0))
    for p in list(lin.parameters()) + list(bn.parameters()):
        p.grad = torch.randn_like(p)
    for _ in range(2):
        rows = osd._rows(w)
        assert len(rows) == 6
        tensors, grads, index, scalars, flags, undo = osd._plan(w, rows)
        assert len(tensors) == 6 and sum(g is not None for g in grads) == 4 and scalars.dtype == np.float32 and scalars.shape[1] == 8
    assert all(pg["weight_decay"] == 0 for pg in w.opt.param_groups)
    osd._plan(w, osd._rows(w))[5]()                                # a third plan and its undo: the counts are back at 2
    assert float(w.opt.state[lin.weight]["step"]) == 2
    for p in idle.parameters():
        assert len(w.opt.state[p]) == 0                           # no gradient: no state, no step count
    for p in lin.parameters():
        st = w.opt.state[p]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"]
        assert st["step"].dtype == torch.float32 and st["step"].ndim == 0 and st["step"].device.type == "cpu" and float(st["step"]) == 2
        assert st["exp_avg"].shape == p.shape and st["exp_avg"].dtype == torch.float32
    # ... it loads into a fresh optimiser of the same structure, whose own step then runs from it
    fresh = make_wrapper(list(lin.parameters()) + list(idle.parameters()), bn.parameters())
    fresh.load_state_dict(w.state_dict())
    fresh.hyper(*onecycle(1))
    before = lin.weight.detach().clone()
    fresh.step()
    assert float(fresh.opt.state[lin.weight]["step"]) == 3 and not torch.equal(before, lin.weight)


def test_refusals_and_hand_overs_that_need_no_gpu():
    from optim_step_cases import Wrapper
    lin = torch.nn.Linear(4, 3)
    for p in lin.parameters():
        p.grad = torch.ones_like(p)
    # parameters on the host reach the method that was replaced, whatever their options: the reference's step takes them
    bound = type("Bound", (Wrapper,), {"step": lambda self: "the replaced step"})
    osd.bind(bound)
    try:
        assert bound.__dict__["step"] is osd.step
        for kw in (dict(), dict(amsgrad=True), dict(maximize=True)):
            w = make_wrapper(lin.parameters(), [], cls=bound, **kw)
            assert w.step() == "the replaced step" and len(w.opt.state) == 0
        half = torch.nn.Linear(4, 3).half()
        assert make_wrapper(half.parameters(), [], cls=bound).step() == "the replaced step"
    finally:
        osd.unbind(bound)
    with pytest.raises(NotImplementedError, match="replaced no method"):
        osd.step(make_wrapper(lin.parameters(), []))                      # never bound: nothing to hand the call to
    # host tensors, another norm type and error_if_nonfinite reach torch's own function
    norm = osd.clip_grad_norm_(iter(lin.parameters()), 1.0)
    assert norm.device.type == "cpu" and abs(float(norm) - math.sqrt(15)) < 1e-5
    assert abs(float(lin.weight.grad[0, 0]) - 1 / math.sqrt(15)) < 1e-6
    assert float(osd.clip_grad_norm_(lin.weight, 10.0, norm_type=1)) == pytest.approx(12 / math.sqrt(15), rel=1e-5)
    lin.weight.grad[0, 0] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        osd.clip_grad_norm_(lin.parameters(), 1.0, error_if_nonfinite=True)
    assert float(osd.clip_grad_norm_([torch.nn.Parameter(torch.zeros(2))], 1.0)) == 0.0     # no gradient: what torch returns
