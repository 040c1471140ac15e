"""Exact nearest-neighbour search between two stored sets: for every row of `x` its k nearest rows of `y`, as
(distance, index) pairs - what a memorisation audit (the nearest training clips of every generated clip), a per-sample
inspection or a nearest-neighbour ratio test asks for once FAD, KAD and PRDC are reported.  The reference has no such
function; its PRDC keeps only the distance of the (k+1)-th neighbour (prdc.py:4-14).

  d2(a, b) = max(fmaf(-2, a.b, |a|^2 + |b|^2), 0)      f32, the arithmetic of the exact k-NN kernel behind prdc()

so the distances are the very values the radii were taken from (column k of a (k + 1)-search is the radius of
nearest_k = k, bit for bit), and no N x M matrix exists at any time (ops.knn_search).

Windows of tracks.  The embedding pipeline cuts every file into windows, so the nearest stored row of almost every window
is a sibling window of its own song, and skipping "the row itself" does not help.  With `groups` (one integer label per
stored row: the song a window comes from) a row's neighbours are the nearest rows WITH ANOTHER LABEL
(ops.knn_search_groups): the whole song is left out, the row included."""
import numpy as np
import torch

from .. import hip_ops as ops
from ..data import AudioMetricsData
from ._groups import joint_group_ids, labelled_rows


def _rows_of(data, name):
    rows = getattr(data, "embeddings", None)
    if rows is None or rows.shape[0] == 0:
        raise ValueError(f"nearest_neighbors needs the stored rows of its {name} set, which keeps none "
                         f"(store_embeddings={getattr(data, 'store_embeddings', None)})")
    if rows.dtype == torch.float64:
        raise NotImplementedError(f"nearest_neighbors: the {name} set holds float64 rows; knn_search takes float32 rows "
                                  "(the float64 matrix-core form is not implemented)")
    return rows


def nearest_neighbors(x: AudioMetricsData, y: AudioMetricsData, k=1, exclude_self=False, squared=False, groups=None,
                      searched_groups=None):
    """The k nearest stored rows of `y` for every stored row of `x`.  Returns {"nn_distances": float32 numpy [n, k],
    "nn_indices": int64 numpy [n, k]} in stored row order of x, neighbours ascending by distance, indices naming stored
    rows of y; one read-back.  Ties go to the smallest index.  exclude_self=True (requires `x is y`) skips each row itself -
    by index, so duplicates of a row remain its neighbours at distance 0.  Where a row has fewer than k finite candidates
    (y smaller than k, rows with non-finite elements) the trailing entries are (+inf, -1).  float32 rows, 1 <= k <= 32.
    squared=True returns the squared distances.  This is a per-row result, not a row of AudioMetrics.evaluate(), which
    returns scalars.

    groups / searched_groups: one integer label per stored row of x / of y (any integer dtype, host or device, any order;
    the song a window comes from).  A row of y whose label EQUALS the label of the row of x is skipped - labels are compared
    by value across the two sets - so a set searched against itself with its labels leaves each row's whole song out.  With
    `x is y` searched_groups defaults to groups; otherwise both are required.  exclude_self=True together with groups raises
    ValueError: the group already contains the row.  PASS LABELS WHENEVER THE ROWS ARE WINDOWS OF TRACKS and the question is
    about other tracks."""
    k = int(k)
    if not 1 <= k <= ops.KNN_SEARCH_MAX_K:
        raise ValueError(f"k={k} must be in 1 .. {ops.KNN_SEARCH_MAX_K}")
    if exclude_self and x is not y:
        raise ValueError("exclude_self=True skips row i of a set searched against itself: it needs x is y")
    grouped = groups is not None or searched_groups is not None
    if grouped:
        if exclude_self:
            raise ValueError("exclude_self=True together with groups: a row's group already contains the row")
        if groups is None:
            raise ValueError("searched_groups without groups: the rows of x need labels to be compared with")
        if searched_groups is None:
            if x is not y:
                raise ValueError("groups without searched_groups: two different sets need the labels of both (with x is y "
                                 "searched_groups defaults to groups)")
            searched_groups = groups
    ex = _rows_of(x, "query")
    ey = ex if x is y else _rows_of(y, "searched")
    if ex.shape[1] != ey.shape[1]:
        raise ValueError(f"feature widths differ: {ex.shape[1]} and {ey.shape[1]}")
    if grouped:
        _, _, lx = labelled_rows(x, groups, "nearest_neighbors", "its query set")
        _, _, ly = labelled_rows(y, searched_groups, "nearest_neighbors", "its searched set")
        gx, gy = joint_group_ids(lx, ly, ex.device)
        dist, idx = ops.knn_search_groups(ex, ey, k, gx, gy, squared=squared)
    else:
        dist, idx = ops.knn_search(ex, ey, k, self_offset=0 if exclude_self else None, squared=squared)
    # the one read-back: the float32 bit patterns travel beside the indices as int64 [n, 2 k]
    both = torch.cat([dist.view(torch.int32).to(torch.int64), idx], dim=1).cpu().numpy()
    return {"nn_distances": both[:, :k].astype(np.int32).view(np.float32), "nn_indices": both[:, k:].copy()}
