"""tests/golden/kitti_eval.npz (tools/make_golden_eval.py: the reference's own eval.py) as annos and overlap blocks."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_eval.npz")
KEYS = ("truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")


def load():
    z = np.load(GOLD)
    out = {"z": z}
    for tag in ("gt", "dt"):
        n = z[f"{tag}_n"]
        off = np.concatenate([[0], np.cumsum(n)])
        annos = []
        for f in range(len(n)):
            s, e = off[f], off[f + 1]
            a = {"name": np.array(z[f"{tag}_name"][s:e].tolist())}
            for k in KEYS:
                if f"{tag}_{k}" in z:
                    a[k] = z[f"{tag}_{k}"][s:e].copy()
            if "score" not in a:
                a["score"] = np.zeros(e - s)
            annos.append(a)
        out[tag] = annos
    bev, d3, o = [], [], 0
    for g, d in zip(out["gt"], out["dt"]):
        k = len(d["name"]) * len(g["name"])
        bev.append(z["bev"][o:o + k].reshape(len(d["name"]), len(g["name"])))
        d3.append(z["d3"][o:o + k].reshape(len(d["name"]), len(g["name"])))
        o += k
    out["bev"], out["d3"] = bev, d3
    for tag in ("range", "car", "ped"):
        out[tag] = (str(z[f"{tag}_str"]), dict(zip(z[f"{tag}_keys"].tolist(), z[f"{tag}_vals"].tolist())))
    return out
