"""tests/golden/kitti_infos.npz (tools/make_golden_infos.py) as KITTI-format trees, and the comparison the infos tests
share: nested dicts / lists equal with the same keys in the same order, the same types, dtypes and shapes, values bit for
bit."""
import hashlib
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TREES = ("dyn", "car")


def golden():
    return np.load(os.path.join(GOLD, "kitti_infos.npz"))


# ---- nested python / numpy objects <-> a JSON skeleton + a list of arrays ----------------------------------------------
def encode(obj, arrays):
    if isinstance(obj, dict):
        return {"d": [[encode(k, arrays), encode(v, arrays)] for k, v in obj.items()]}
    if isinstance(obj, (list, tuple)):
        return {"l" if isinstance(obj, list) else "t": [encode(v, arrays) for v in obj]}
    if isinstance(obj, np.str_):
        return {"S": str(obj)}
    if isinstance(obj, np.ndarray) and obj.dtype.kind == "U":
        return {"U": [str(x) for x in obj.ravel()], "shape": list(obj.shape), "dtype": obj.dtype.str}
    if isinstance(obj, (np.ndarray, np.generic)):
        arrays.append(np.asarray(obj))
        return {"a": len(arrays) - 1, "scalar": isinstance(obj, np.generic)}
    assert obj is None or isinstance(obj, (str, int, float, bool)), type(obj)
    return {"p": obj, "type": type(obj).__name__}


def decode(sk, arrays):
    if "d" in sk:
        return {decode(k, arrays): decode(v, arrays) for k, v in sk["d"]}
    if "l" in sk:
        return [decode(v, arrays) for v in sk["l"]]
    if "t" in sk:
        return tuple(decode(v, arrays) for v in sk["t"])
    if "S" in sk:
        return np.str_(sk["S"])
    if "U" in sk:
        return np.array(sk["U"], dtype=sk["dtype"]).reshape(sk["shape"])
    if "a" in sk:
        a = arrays[sk["a"]]
        return a[()] if sk["scalar"] else a
    return sk["p"]


def store(out, key, obj):
    arrays = []
    out[key + "/json"] = np.array(json.dumps(encode(obj, arrays)))
    for i, a in enumerate(arrays):
        out["%s/%d" % (key, i)] = a


def fetch(g, key):
    sk = json.loads(str(g[key + "/json"]))
    n = 0
    while "%s/%d" % (key, n) in g.files:
        n += 1
    return decode(sk, [g["%s/%d" % (key, i)] for i in range(n)])


def assert_same(a, b, where="root"):
    assert type(a) is type(b), (where, type(a), type(b))
    if isinstance(a, dict):
        assert list(a.keys()) == list(b.keys()), (where, list(a.keys()), list(b.keys()))
        for (ka, va), (kb, vb) in zip(a.items(), b.items()):
            assert type(ka) is type(kb), (where, ka)
            assert_same(va, vb, "%s[%r]" % (where, ka))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), (where, len(a), len(b))
        for i, (va, vb) in enumerate(zip(a, b)):
            assert_same(va, vb, "%s[%d]" % (where, i))
    elif isinstance(a, (np.ndarray, np.generic)):
        assert a.dtype == b.dtype and a.shape == b.shape, (where, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype.kind in "US":
            assert np.array_equal(a, b), where
        else:
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (where, a, b)
    else:
        assert a == b, (where, a, b)


# ---- the trees --------------------------------------------------------------------------------------------------------
def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def tree_scans(g, name):
    """[(idx, rows (n,4) float32, label text, calib text, (W, H))]: the base points come from modest_amd.synth (seeded, no
    libm), the planted rows from the fixture; the digest of every scan's bytes is checked against the fixture"""
    from modest_amd import synth
    ids = [str(x) for x in g[name + "/ids"]]
    labels, calibs = [str(x) for x in g[name + "/labels"]], [str(x) for x in g[name + "/calibs"]]
    eo, extras = g[name + "/extra_offsets"], g[name + "/extras"]
    out = []
    for k, idx in enumerate(ids):
        base = synth.infos_points(int(g[name + "/seeds"][k]), labels[k], int(g[name + "/n_bg"][k]), (50, 2000))
        rows = np.ascontiguousarray(np.concatenate([base, extras[eo[k]:eo[k + 1]]]), dtype=np.float32)
        assert sha(rows.tobytes()) == str(g[name + "/bin_sha"][k]), "synthetic scan %s differs from the recorded one" % idx
        out.append((idx, rows, labels[k], calibs[k], tuple(int(v) for v in g[name + "/sizes"][k])))
    return out


def write_tree(g, name, root):
    from modest_amd import synth
    scans = tree_scans(g, name)
    for idx, rows, label, calib, size in scans:
        synth.write_infos_scan(str(root), idx, rows, label, calib, size)
    synth.write_infos_splits(str(root), [str(x) for x in g[name + "/train"]], [str(x) for x in g[name + "/val"]])
    return scans


def expected(g, name, fov=True):
    """(infos_train, infos_val, dbinfos) of the reference; fov=False: its counts with FOV_POINTS_ONLY off"""
    tr, va, db = fetch(g, name + "/infos_train"), fetch(g, name + "/infos_val"), fetch(g, name + "/dbinfos")
    if not fov:
        for split, infos in (("train", tr), ("val", va)):
            alt = fetch(g, name + "/counts_nofov_" + split)
            for info, c in zip(infos, alt):
                info["annos"]["num_points_in_gt"] = c
    return tr, va, db


def check_outputs(g, name, root, fov=True, val=True):
    """the files under `root` against the fixture: pickles equal after load, database files byte for byte"""
    import pickle
    tr, va, db = expected(g, name, fov)
    load = lambda f: pickle.load(open(os.path.join(str(root), f), "rb"))   # noqa: E731
    assert_same(load("kitti_infos_train.pkl"), tr, "train")
    if val:
        assert_same(load("kitti_infos_val.pkl"), va, "val")
    assert_same(load("kitti_dbinfos_train.pkl"), db, "dbinfos")
    names = [str(x) for x in g[name + "/db_names"]]
    assert sorted(os.listdir(os.path.join(str(root), "gt_database"))) == sorted(names)
    for f, n, h in zip(names, g[name + "/db_counts"], g[name + "/db_sha"]):
        data = open(os.path.join(str(root), "gt_database", f), "rb").read()
        assert len(data) == 16 * int(n), (f, len(data) // 16, int(n))
        assert sha(data) == str(h), f
