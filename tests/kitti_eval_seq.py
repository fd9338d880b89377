"""A sequential restatement of eval.py's statistics and AP logic (kitti_object_eval_python/eval.py), in plain Python
over precomputed per-frame overlap blocks.  The tests pin it to the reference's recorded outputs and then use it as
the yardstick of the device statistics."""
import numpy as np

from modest_amd import kitti_eval as ke

NO_DETECTION = -10000000


def compute_statistics(ov, gt_alpha, dt_alpha, dt_bbox, dt_score, ignored_gt, ignored_det, dc_bboxes, metric,
                       min_overlap, thresh=0.0, compute_fp=False, compute_aos=False):
    """eval.py:160-278.  ov: (dt, gt) block."""
    nd, ng = len(ignored_det), len(ignored_gt)
    assigned = [False] * nd
    below = [compute_fp and dt_score[j] < thresh for j in range(nd)]
    tp = fp = fn = 0
    similarity = 0
    tp_scores, delta = [], []
    for i in range(ng):                                   # gt in order: assigned_detection persists
        if ignored_gt[i] == -1:
            continue
        det_idx, valid, max_overlap, took_ignored = -1, NO_DETECTION, 0, False
        for j in range(nd):
            if ignored_det[j] == -1 or assigned[j] or below[j]:
                continue
            o, s = ov[j, i], dt_score[j]
            if not compute_fp and o > min_overlap and s > valid:            # pass A: highest score, first wins ties
                det_idx, valid = j, s
            elif compute_fp and o > min_overlap and (o > max_overlap or took_ignored) and ignored_det[j] == 0:
                max_overlap, det_idx, valid, took_ignored = o, j, 1, False   # pass B: first max overlap
            elif compute_fp and o > min_overlap and valid == NO_DETECTION and ignored_det[j] == 1:
                det_idx, valid, took_ignored = j, 1, True                     # else the first ignored detection
        if valid == NO_DETECTION and ignored_gt[i] == 0:
            fn += 1
        elif valid != NO_DETECTION and (ignored_gt[i] == 1 or ignored_det[det_idx] == 1):
            assigned[det_idx] = True
        elif valid != NO_DETECTION:
            tp += 1
            tp_scores.append(dt_score[det_idx])
            if compute_aos:
                delta.append(gt_alpha[i] - dt_alpha[det_idx])
            assigned[det_idx] = True
    if compute_fp:
        for j in range(nd):
            if not (assigned[j] or ignored_det[j] == -1 or ignored_det[j] == 1 or below[j]):
                fp += 1
        nstuff = 0
        if metric == 0 and len(dc_bboxes):                 # eval.py:252-265: DontCare boxes take unmatched detections
            odc = ke.image_box_overlap(dt_bbox, np.asarray(dc_bboxes), 0)
            for i in range(len(dc_bboxes)):
                for j in range(nd):
                    if assigned[j] or ignored_det[j] in (-1, 1) or below[j]:
                        continue
                    if odc[j, i] > min_overlap:
                        assigned[j] = True
                        nstuff += 1
        fp -= nstuff
        if compute_aos:
            if tp > 0 or fp > 0:
                similarity = 0.0
                for d in delta:                           # numba's np.sum: in order from zero
                    similarity += (1.0 + np.cos(d)) / 2.0
            else:
                similarity = -1
    return tp, fp, fn, similarity, tp_scores


def get_thresholds_loop(scores, num_gt, num_sample_pts=41):
    """eval.py:10-28 as written"""
    scores = np.sort(scores)[::-1]
    current_recall, thresholds = 0, []
    for i, score in enumerate(scores):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < len(scores) - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < len(scores) - 1:
            continue
        thresholds.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


def frame_flags(g, d, cls, diff):
    n_valid, ig, idt, dc = ke.clean_data(g, d, cls, diff)
    return n_valid, ig, idt, dc


def eval_config(frames, metric, cls, diff, min_overlap, compute_aos=False, flags=None):
    """one configuration over frames [(gt anno, dt anno, (dt, gt) overlap block)] -> pr table (T, 4), thresholds"""
    prep = []
    nvalid = 0
    for k, (g, d, ov) in enumerate(frames):
        n, ig, idt, dc = flags[k] if flags is not None else frame_flags(g, d, cls, diff)
        nvalid += n
        prep.append((g, d, ov, ig, idt, dc))
    scores = []
    for g, d, ov, ig, idt, dc in prep:
        scores += compute_statistics(ov, g["alpha"], d["alpha"], d["bbox"], d["score"], ig, idt, dc, metric,
                                     min_overlap)[4]
    thr = get_thresholds_loop(np.array(scores), nvalid) if scores else []
    pr = np.zeros((len(thr), 4))
    for g, d, ov, ig, idt, dc in prep:
        for t, s in enumerate(thr):
            tp, fp, fn, sim, _ = compute_statistics(ov, g["alpha"], d["alpha"], d["bbox"], d["score"], ig, idt, dc,
                                                    metric, min_overlap, s, True, compute_aos)
            pr[t, 0] += tp
            pr[t, 1] += fp
            pr[t, 2] += fn
            if sim != -1:
                pr[t, 3] += sim
    return pr, np.array(thr)


def curves(pr, compute_aos):
    rec, prec, aos = np.zeros(41), np.zeros(41), np.zeros(41)
    with np.errstate(divide='ignore', invalid='ignore'):
        for i in range(len(pr)):
            rec[i] = pr[i, 0] / (pr[i, 0] + pr[i, 2])
            prec[i] = pr[i, 0] / (pr[i, 0] + pr[i, 1])
            if compute_aos:
                aos[i] = pr[i, 3] / (pr[i, 0] + pr[i, 1])
        for i in range(len(pr)):
            prec[i] = np.max(prec[i:], axis=-1)
            if compute_aos:
                aos[i] = np.max(aos[i:], axis=-1)
    return rec, prec, aos


def in_range(a, close, far):
    z = np.abs(np.asarray(a["location"]).reshape(-1, 3)[:, 2])
    return (z > close) & (z <= far)


def range_flags(frames, cls, rng):
    """difficulty-3 flags with the boxes outside the range marked -1 (and DontCare boxes dropped)"""
    out = []
    for g, d, _ in frames:
        n, ig, idt, dc = ke.clean_data(g, d, cls, 3)
        ing, ind = in_range(g, *rng), in_range(d, *rng)
        ig = [v if ing[i] else -1 for i, v in enumerate(ig)]
        idt = [v if ind[j] else -1 for j, v in enumerate(idt)]
        dcs = [g["bbox"][i] for i in range(len(g["name"])) if g["name"][i] == "DontCare" and ing[i]]
        out.append((int(sum(1 for v in ig if v == 0)), ig, idt, dcs))
    return out


def range_eval(gt, dt, bev, d3, cls_name="Dynamic", ranges=(0, 30, 50, 80)):
    """get_range_eval_result from per-frame (dt, gt) BEV and 3-D blocks"""
    class_to_name = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting', 5: 'Truck', 6: 'Dynamic'}
    cls = {v: k for k, v in class_to_name.items()}[cls_name]
    mo = {1: (0.5, 0.25), 2: (0.5, 0.25)}      # get_range_eval_result's tables, column 6 (Dynamic)
    assert cls == 6, "the restatement covers the Dynamic range eval"
    pairs = [(ranges[i], ranges[i + 1]) for i in range(len(ranges) - 1)] + [[ranges[0], ranges[-1]]]
    ret = {}
    for s, e in pairs:
        res = {}
        for metric, blocks in ((1, bev), (2, d3)):
            frames = list(zip(gt, dt, blocks))
            fl = range_flags(frames, cls, (s, e))
            prec = np.zeros((1, 1, 2, 41))
            for k in range(2):
                pr, _ = eval_config(frames, metric, cls, 3, mo[metric][k], flags=fl)
                prec[0, 0, k] = curves(pr, False)[1]
            res[metric] = ke.get_mAP_R40(prec)
        ret[f'{cls_name}_3d_iou0.7/{s:02d}-{e:02d}_R40'] = res[2][0, 0, 0]
        ret[f'{cls_name}_3d_iou0.5/{s:02d}-{e:02d}_R40'] = res[2][0, 0, 1]
        ret[f'{cls_name}_bev_iou0.7/{s:02d}-{e:02d}_R40'] = res[1][0, 0, 0]
        ret[f'{cls_name}_bev_iou0.5/{s:02d}-{e:02d}_R40'] = res[1][0, 0, 1]
    return ke._range_result_string(ret, [cls], class_to_name, pairs), ret
