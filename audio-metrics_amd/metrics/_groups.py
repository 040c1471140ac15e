"""Row groups of the per-group ("per-song") metrics: one integer label per stored row, turned into the list of groups
rows[order[offsets[b]:offsets[b + 1]]] that hip_ops.frechet_groups / mmd_rbf_group_sums / stats_gather take."""
import numpy as np
import torch


def _group_labels(groups):
    """The labels as a 1-D integer torch tensor (host or device, as given); no device call."""
    if isinstance(groups, torch.Tensor):
        labels = groups
        if labels.dtype == torch.bool or labels.is_floating_point() or labels.is_complex():
            raise ValueError(f"groups must hold integer labels, got dtype {labels.dtype}")
    else:
        arr = np.asarray(groups)
        if arr.size and arr.dtype.kind not in "iu":
            raise ValueError(f"groups must hold integer labels, got dtype {arr.dtype}")
        if arr.dtype.kind == "u" and arr.size and int(arr.max()) > np.iinfo(np.int64).max:
            raise ValueError("groups holds a label beyond the int64 range")
        labels = torch.as_tensor(np.ascontiguousarray(arr.astype(np.int64)))
    if labels.dim() != 1:
        raise ValueError(f"groups must be 1-D (one label per stored row), got shape {tuple(labels.shape)}")
    return labels


def labelled_rows(x, groups, function_name, which_set_words):
    """(stored rows of x, their number, one label per row) after the checks every per-group metric opens with; no device
    call.  which_set_words names x in the message ("its first argument", "its candidate set")."""
    rows = getattr(x, "embeddings", None)
    n = int(rows.shape[0]) if rows is not None else 0
    if rows is None or n == 0:
        raise ValueError(f"{function_name} scores the stored rows of {which_set_words}, which keeps none "
                         f"(store_embeddings={getattr(x, 'store_embeddings', None)})")
    labels = _group_labels(groups)
    if labels.numel() == 0:
        raise ValueError("groups is empty")
    if labels.numel() != n:
        raise ValueError(f"groups holds {labels.numel()} labels for {n} stored rows (one label per row)")
    return rows, n, labels


def sort_into_groups(labels):
    """(order, counts, group_labels, sizes) of int64 labels on a device: `order` lists the rows group by group in
    ascending label order (stable inside a group), `counts` the group sizes on the device; group_labels and sizes are
    the host copies, from the one read-back in front of the kernels."""
    sorted_labels, order = torch.sort(labels, stable=True)
    uniq, counts = torch.unique_consecutive(sorted_labels, return_counts=True)
    host = torch.stack([uniq, counts]).cpu().numpy()
    return order, counts, host[0].copy(), host[1].astype(np.int64)


def joint_group_ids(labels_x, labels_y, device):
    """Dense int32 ids of two label vectors ON `device`, mapped JOINTLY so that equal labels of the two sets get equal
    ids (hip_ops.knn_search_groups compares ids across the sets): one torch.unique over both, no read-back."""
    both = torch.cat([labels_x.to(device=device, dtype=torch.int64), labels_y.to(device=device, dtype=torch.int64)])
    inverse = torch.unique(both, return_inverse=True)[1].to(torch.int32)
    return inverse[:labels_x.numel()].contiguous(), inverse[labels_x.numel():].contiguous()
