"""Precision / recall / density / coverage and per-sample fidelity with the SONG as the unit: leave-group-out k-NN radii
and a membership pass that skips the pairs of equal labels.  The reference has no such functions.

The rows this package scores are windows of tracks, so stored rows come in runs of near-duplicates per song.  The k-NN
radius of a window is then the distance to a sibling window of its own song and the "manifold" a set of song-sized specks:
two sets of DIFFERENT songs drawn from one distribution score precision = recall = 0.  With `groups` (one integer label
per stored row: the song) the radius of a row is the distance to its k-th nearest row WITH ANOTHER LABEL
(ops.knn_search_groups).  That alone is not enough where the two sets share songs - the accompaniment setting, candidate
and reference rendered over the same contexts: a window lies inside the now wider balls of its own song's windows in the
other set whatever the model did, and precision saturates at 1.  So the membership pass knows the labels as well
(ops.sample_scores_groups): with "admissible" = different labels, compared by VALUE across the two sets,

  precision  mean over candidate rows of [count > 0],  count = #{ admissible reference rows j : d < r_ref[j] }
  density    (1 / k) * mean count
  recall     mean over reference rows of [#{ admissible candidate rows i : d < r_cand[i] } > 0]
  coverage   mean over reference rows of [distance to the nearest admissible candidate row < r_ref[j]], strict, float32;
             a row with no admissible candidate is not covered

on the integers and expressions of metrics/prdc.py.  match_across_sets=False compares labels only INSIDE each set (two sets
with unrelated label spaces): the same radii, every cross-set pair counts, and the counts come from ops.prdc_counts.  With
label values that no row of the other set carries the two settings agree exactly.

Labels: any integer dtype, host or device, any order (_groups.labelled_rows), mapped jointly to dense int32 ids on the
device (_groups.joint_group_ids).  float32 rows; no process_group sharding; none of this is a metric of
AudioMetrics.evaluate()."""
import numpy as np
import torch

from .. import hip_ops as ops
from ._groups import joint_group_ids, labelled_rows


def check_nearest_k(nearest_k):
    k = int(nearest_k)
    if not 1 <= k <= ops.KNN_SEARCH_MAX_K:
        raise ValueError(f"nearest_k={k} must be in 1 .. {ops.KNN_SEARCH_MAX_K} (the leave-group-out radii come from the k-NN search)")
    return k


def labelled_f32_rows(data, groups, function_name, which_set_words):
    """labelled_rows plus the float32 check; no device call."""
    rows, n, labels = labelled_rows(data, groups, function_name, which_set_words)
    if rows.dtype == torch.float64:
        raise NotImplementedError(f"{function_name}: {which_set_words} holds float64 rows; the leave-group-out sweeps take float32 "
                                  "rows (the float64 matrix-core form is not implemented)")
    return rows, n, labels


def require_rows_outside_every_group(labels, k, function_name, which_set_words):
    """ValueError when some label leaves fewer than k rows outside it: such a row's radius would be +inf and its ball
    everything.  Decided from the label counts on the host, in front of the kernels (labels that live on a device cost
    one scalar read-back here)."""
    if labels.device.type == "cpu":
        largest = int(np.unique(labels.numpy(), return_counts=True)[1].max())
    else:
        largest = int(torch.unique(labels, return_counts=True)[1].max())
    n = int(labels.numel())
    if n - largest < k:
        raise ValueError(f"{function_name}: a label of {which_set_words} holds {largest} of its {n} rows and leaves {n - largest} "
                         f"outside it, fewer than nearest_k={k}: its rows have no leave-group-out radius")


def _own_ids(labels, device):
    return torch.unique(labels.to(device=device, dtype=torch.int64), return_inverse=True)[1].to(torch.int32).contiguous()


def radii_from_ids(rows, ids, k):
    """Column k - 1 of the leave-group-out search of a set against itself: the k-th and not the (k + 1)-th, because the row
    sits inside its own group."""
    return ops.knn_search_groups(rows, rows, k, ids, ids)[0][:, k - 1].contiguous()


def leave_group_out_radii(data, groups, nearest_k):
    """Device float32 [rows]: the distance of every stored row of `data` to its nearest_k-th nearest stored row WITH
    ANOTHER LABEL (ops.knn_search_groups of the set against itself; 1 <= nearest_k <= 32).  With one label per row it is
    data.get_radii(nearest_k) bit for bit.  ValueError, before any kernel, when some label leaves fewer than nearest_k rows
    outside it.  Not cached on the set: prdc_leave_group_out takes ref_radii= / cand_radii= for callers who score many
    candidates against one reference."""
    k = check_nearest_k(nearest_k)
    rows, _, labels = labelled_f32_rows(data, groups, "leave_group_out_radii", "its set")
    require_rows_outside_every_group(labels, k, "leave_group_out_radii", "its set")
    return radii_from_ids(rows, _own_ids(labels, rows.device), k)


def _given_radii(radii, n, name):
    if not torch.is_tensor(radii) or radii.dtype != torch.float32 or radii.dim() != 1 or radii.shape[0] != n:
        raise ValueError(f"{name} must be a float32 tensor with one radius per stored row ({n}), got "
                         f"{(tuple(radii.shape), radii.dtype) if torch.is_tensor(radii) else type(radii).__name__}")
    return radii


def prdc_leave_group_out(reference, candidate, nearest_k, ref_groups, groups, match_across_sets=True, ref_radii=None,
                         cand_radii=None, return_rows=False):
    """precision, recall, density, coverage (Python floats) of `candidate` against `reference` with leave-group-out radii on
    both sides and - match_across_sets=True - only the pairs of DIFFERENT labels as pairs (module docstring), plus
    nearest_k and shared_labels: the number of label values present in both sets, so that a caller who reused 0 .. B on
    both sides by accident sees it.  ref_groups / groups: one integer label per stored row of reference / of candidate.
    ref_radii / cand_radii: what leave_group_out_radii returned for that set and nearest_k (then the set is not searched
    again).  return_rows=True adds candidate_ball_count (int32 [n]), reference_recalled and reference_covered (bool [m]) in
    stored row order.  One read-back."""
    name = "prdc_leave_group_out"
    k = check_nearest_k(nearest_k)
    if ref_groups is None or groups is None:
        raise ValueError(f"{name} needs the labels of both sets (ref_groups and groups): one integer label per stored row")
    ey, m, ly = labelled_f32_rows(reference, ref_groups, name, "its reference set")
    ex, n, lx = labelled_f32_rows(candidate, groups, name, "its candidate set")
    if ex.shape[1] != ey.shape[1]:
        raise ValueError(f"feature widths differ: {ey.shape[1]} and {ex.shape[1]}")
    if ref_radii is not None:
        ref_radii = _given_radii(ref_radii, m, "ref_radii")
    else:
        require_rows_outside_every_group(ly, k, name, "its reference set")
    if cand_radii is not None:
        cand_radii = _given_radii(cand_radii, n, "cand_radii")
    else:
        require_rows_outside_every_group(lx, k, name, "its candidate set")
    gx, gy = joint_group_ids(lx, ly, ex.device)
    r_ref = radii_from_ids(ey, gy, k) if ref_radii is None else ref_radii.contiguous()
    r_cand = radii_from_ids(ex, gx, k) if cand_radii is None else cand_radii.contiguous()
    if match_across_sets:
        count = ops.sample_scores_groups(ex, ey, r_ref, gx, gy)[2]
        recalled = ops.sample_scores_groups(ey, ex, r_cand, gy, gx)[2] > 0
        nearest = ops.knn_search_groups(ey, ex, 1, gy, gx)[0][:, 0]
        covered = nearest < r_ref                                   # strict, f32; +inf (no admissible candidate) is not below anything
    else:
        count, row_any, row_cover = ops.prdc_counts(ey, ex, r_ref, r_cand)
        recalled, covered = row_any != 0, row_cover != 0
    shared = torch.isin(torch.unique(gx), gy).sum()
    count64 = count.to(torch.int64)
    parts = [torch.stack([(count64 > 0).sum(), recalled.sum(), count64.sum(), covered.sum(), shared])]
    if return_rows:
        parts += [count64, recalled.to(torch.int64), covered.to(torch.int64)]
    host = torch.cat(parts).cpu().numpy()                          # the one read-back
    n_prec, n_rec, sum_cnt, n_cov, n_shared = (int(v) for v in host[:5])
    # the expressions of metrics/prdc.py on the same integers
    out = dict(precision=n_prec / n, recall=n_rec / m, density=(1.0 / float(k)) * (sum_cnt / n), coverage=n_cov / m,
               nearest_k=k, shared_labels=n_shared)
    if return_rows:
        out["candidate_ball_count"] = host[5:5 + n].astype(np.int32)
        out["reference_recalled"] = host[5 + n:5 + n + m].astype(bool)
        out["reference_covered"] = host[5 + n + m:5 + n + 2 * m].astype(bool)
    return out


def grouped_scores(function_name, samples, ex, manifold, ey, k, groups, manifold_groups, match_across_sets):
    """What sample_fidelity runs once a label keyword is given: the five device tensors.  The radii are the
    leave-group-out radii of the manifold; with sample labels as well and matching on, the pass is
    ops.sample_scores_groups, else ops.sample_scores with those radii.  Validation first, no device call before it."""
    check_nearest_k(k)
    if groups is not None and manifold_groups is None:
        if samples is not manifold:
            raise ValueError(f"{function_name}: groups without manifold_groups: two different sets need the labels of both (with "
                             "samples is manifold manifold_groups defaults to groups)")
        manifold_groups = groups
    _, _, ly = labelled_f32_rows(manifold, manifold_groups, function_name, "its manifold set")
    lx = None
    if groups is not None:
        lx = ly if (samples is manifold and manifold_groups is groups) else \
            labelled_f32_rows(samples, groups, function_name, "its sample set")[2]
    require_rows_outside_every_group(ly, k, function_name, "its manifold set")
    if lx is not None and match_across_sets:
        gx, gy = joint_group_ids(lx, ly, ey.device)
        return ops.sample_scores_groups(ex, ey, radii_from_ids(ey, gy, k), gx, gy)
    return ops.sample_scores(ex, ey, radii_from_ids(ey, _own_ids(ly, ey.device), k))


def grouped_authenticity(function_name, g, gen, x, train, train_groups, groups):
    """What authenticity_score runs once train_groups is given: (dist [M], idx [M], radii [N]) on the device.  A training
    row's own-set neighbour distance leaves its group out; with `groups` the nearest training row of a generated row is
    searched among the other labels."""
    if train_groups is None:
        raise ValueError(f"{function_name}: groups without train_groups: the training rows need labels to be compared with")
    _, _, lt = labelled_f32_rows(train, train_groups, function_name, "its training set")
    lg = None if groups is None else labelled_f32_rows(gen, groups, function_name, "its generated set")[2]
    require_rows_outside_every_group(lt, 1, function_name, "its training set")
    if lg is None:
        radii = radii_from_ids(x, _own_ids(lt, x.device), 1)
        dist, idx = ops.knn_search(g, x, 1)
    else:
        gg, gt = joint_group_ids(lg, lt, x.device)
        radii = radii_from_ids(x, gt, 1)
        dist, idx = ops.knn_search_groups(g, x, 1, gg, gt)
    return dist[:, 0], idx[:, 0], radii
