"""Cases of the optimiser-step tests: the reader of tests/golden/optim_step.npz, a stand-in for the
reference's OptimWrapper with the attributes the drop-in reads, a OneCycle list, and the named tensor sets."""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "optim_step.npz")
SHAPES = os.path.join(HERE, "golden", "optim_step_shapes.json")
CH = 4096
SIZES = (0, 1, 3, 4, 5, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 7)


def scenes():
    """-> {scene: [step]}; a step: tensors (group order; dicts with name, p, g, gc, m, v, t before and p1, m1, v1, t1 after, lr,
    beta1, beta2, eps, wd, dec, bn, frozen), model_order, norm (torch's), max_norm"""
    z = np.load(GOLD)
    metas = json.loads(str(z["meta"]))
    out = {}
    for name, meta in metas.items():
        cur = {pr["name"]: dict(p=z[f"{name}.init.{pr['name']}.p"], m=None, v=None, t=0.0) for pr in meta["params"]}
        steps = []
        for k, st in enumerate(meta["steps"]):
            tensors = []
            for pr in meta["params"]:
                n = pr["name"]
                key = f"{name}.{k}.{n}"
                frozen = n in st["frozen"]
                decays = (not pr["bn"] or meta["bn_wd"]) and not frozen
                x = dict(cur[n], name=n, bn=pr["bn"], frozen=frozen, lr=st["lr"], beta1=st["mom"], beta2=st["beta2"], eps=st["eps"],
                         wd=st["wd"], dec=1 - st["wd"] * st["lr"] if decays else 1.0,
                         g=z[key + ".g"] if key + ".g" in z else None, gc=z[key + ".gc"] if key + ".gc" in z else None,
                         p1=z[key + ".p"], m1=z[key + ".m"] if key + ".m" in z else None,
                         v1=z[key + ".v"] if key + ".v" in z else None, t1=st["t"].get(n, 0.0))
                tensors.append(x)
                cur[n] = dict(p=x["p1"], m=x["m1"], v=x["v1"], t=x["t1"])
            steps.append(dict(tensors=tensors, model_order=meta["model_order"], norm=z[f"{name}.{k}.norm"], max_norm=st["max_norm"]))
        out[name] = steps
    return out


def shape_sets():
    with open(SHAPES) as f:
        return json.load(f)


def onecycle(k, total=20, lr_max=0.003, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4):
    """(lr, mom) of step k of a one-cycle schedule: cosine from lr_max / div to lr_max over the first pct_start of the steps and
    down to lr_max / div / 1e4 after; the momentum the other way round"""
    def cos(start, end, pct):
        return end + (start - end) / 2 * (math.cos(math.pi * pct) + 1)
    a = int(total * pct_start)
    low = lr_max / div_factor
    if k < a:
        return cos(low, lr_max, k / a), cos(moms[0], moms[1], k / a)
    return cos(lr_max, low / 1e4, (k - a) / (total - a)), cos(moms[1], moms[0], (k - a) / (total - a))


class Wrapper:
    """What the drop-in reads of the reference's OptimWrapper: opt, true_wd, bn_wd, _lr, _wd, set_val, and the pass-throughs a
    training script uses.  The groups come in pairs: (others, batch norm)."""

    def __init__(self, opt, wd, true_wd=True, bn_wd=True):
        self.opt, self.true_wd, self.bn_wd = opt, true_wd, bn_wd
        pairs = len(opt.param_groups) // 2
        self._lr = [pg["lr"] for pg in opt.param_groups[::2]]
        self._wd = [wd] * pairs

    def set_val(self, key, val):
        for v, pg1, pg2 in zip(val, self.opt.param_groups[::2], self.opt.param_groups[1::2]):
            pg1[key] = pg2[key] = v
        return val

    def hyper(self, lr, mom):
        self._lr = self.set_val("lr", [lr] * len(self._lr))
        beta2 = self.opt.param_groups[0]["betas"][1]
        self.set_val("betas", [(mom, beta2)] * len(self._lr))

    def step(self):
        """the method the drop-in replaces: decay, then the inner optimiser"""
        for lr, wd, pg1, pg2 in zip(self._lr, self._wd, self.opt.param_groups[::2], self.opt.param_groups[1::2]):
            for p in pg1["params"] + (pg2["params"] if self.bn_wd else []):
                if p.requires_grad:
                    p.data.mul_(1 - wd * lr)
        self.set_val("weight_decay", [0] * len(self._wd))
        self.opt.step()

    def zero_grad(self):
        self.opt.zero_grad()

    def state_dict(self):
        return self.opt.state_dict()

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd)

    def clear(self):
        sd = self.state_dict()
        sd["state"] = {}
        self.load_state_dict(sd)


def make_wrapper(others, norms, wd=0.01, betas=(0.9, 0.99), cls=Wrapper, **adam):
    import torch
    opt = torch.optim.Adam([{"params": list(others), "lr": 0}, {"params": list(norms), "lr": 0}], betas=betas, **adam)
    return cls(opt, wd)


def values(n, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal(n) * scale).astype(np.float32)
