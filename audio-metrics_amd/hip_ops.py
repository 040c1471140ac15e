"""Thin torch<->C-ABI glue: device tensors in, device tensors out.

PyTorch is used only as the device-memory allocator and stream owner; every
computation below is a call into libaudio_metrics_hip.so on torch's current
HIP stream.  There is no CPU path: CPU tensors are rejected.

Every operation is written on a few helpers: _rows(e, name, f64) gives a set's matrix form, its leading dimension and the
entry-point suffix; _any_f64 / _both_f64 are the two float64 promotion rules; _refuse_f64, _check_two_sets and _two_sets are
the preamble of the float32 row-sweep ops, _check_gram_rows and _blocks_mask that of the Gram ops; _opt / _host turn optional
tensors / host arrays into pointers; _run(name, dev, query, query_args, *args) asks the workspace query, allocates and calls.
Binding a new entry point am_new_f32 / _f64 with its am_new_workspace_bytes(n, d) takes, after its argument checks:
    rows, ld, kind = _rows(rows, "rows", is_f64(rows))
    out = torch.empty(rows.shape[0], dtype=torch.float64, device=rows.device)
    _run("am_new_" + kind, rows.device, "am_new_workspace_bytes", rows.shape, _ptr(rows), *rows.shape, ld, _opt(weights), _ptr(out))
"""
import ctypes
import math
import struct

import numpy as np
import torch

from . import _lib


def _stream(device=None):
    """torch's current stream ON `device` (the tensors' device, not the thread's current device)."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _opt(t):
    """The device pointer of an optional tensor: NULL for None."""
    return _ptr(t) if t is not None else ctypes.c_void_p(None)


def _host(a):
    """The pointer to a host ctypes array, NULL for None."""
    return ctypes.cast(a, ctypes.c_void_p) if a is not None else ctypes.c_void_p(None)


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


_SIDE_STREAMS = {}


def _side_stream(key, dev):
    """The side stream kept under `key`, created on `dev` at its first use."""
    side = _SIDE_STREAMS.get(key)
    if side is None:
        side = _SIDE_STREAMS[key] = torch.cuda.Stream(dev)
    return side


def upload_host_array(array, device):
    """Host array -> device tensor usable on the current stream, without blocking the host behind the work already
    queued there: the (pageable, host-synchronous) copy is issued on an otherwise idle side stream and the current
    stream waits for it on the device.  Pinned host memory is deliberately NOT used: on this platform both
    `Tensor.pin_memory()` per call and kernels reading a pooled pinned buffer in place stall the host for 75-100 ms
    every few calls (measured on the 2 x 800 KB kernel-distance index tables: a 10 ms evaluate became a 90 ms one every
    third call), while pageable copies of the same data never did."""
    t = torch.as_tensor(np.ascontiguousarray(array))
    if getattr(device, "type", "cpu") != "cuda":
        return t
    main = torch.cuda.current_stream(device)
    side = _side_stream(device.index, device)
    with torch.cuda.stream(side):
        d = t.to(device)
    done = torch.cuda.Event()
    done.record(side)
    main.wait_event(done)
    d.record_stream(main)
    return d


def _index_table(t, name):
    """int64 [S, m] index table on the device."""
    _require_cuda(t, name)
    return t.to(torch.int64).contiguous()


class KernelTimer:
    """Optional per-entry-point timing with HIP events recorded on the stream the
    kernels are launched on (torch's current stream).  Used by bench.py:
        with KernelTimer() as t: ...;  t.summary() -> {name: (calls, total_ms)}"""
    active = None

    def __init__(self):
        self.records = []

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.records:
            c, t = out.get(name, (0, 0.0))
            out[name] = (c + 1, t + a.elapsed_time(b))
        return out


KERNEL_KNN, KERNEL_PRDC_CROSS, KERNEL_KNN_VERIFY, KERNEL_PRDC_VERIFY = 0, 1, 2, 3        # enum am_clocked_kernel


def kernel_clock_enable(on=True):
    """Bracket every launch of the two tile kernels with hipEvents inside the library (bench.py)."""
    _lib.check(_lib.load().am_kernel_clock_enable(1 if on else 0), "am_kernel_clock_enable")


def kernel_clock_read(kernel):
    """(launches, total_ms) of the clocked kernel since the last read; waits for the recorded launches."""
    n, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
    _lib.check(_lib.load().am_kernel_clock_read(int(kernel), ctypes.byref(n), ctypes.byref(ms)), "am_kernel_clock_read")
    return n.value, ms.value


FILTER_STATS_NAMES = ("knn_calls", "knn_queued", "knn_spilled", "knn_verified_pairs", "knn_fallback_rows",
                      "prdc_calls", "prdc_queued", "prdc_overflow_queue", "prdc_fallback_calls", "bound_ratio_max", "bound_pairs")
_FILTER_STATS = {}


def filter_stats_enable(device, on=True):
    """Have the filter-form PRDC entry points add their queue / verification / fallback counts to a device buffer
    (am_filter_stats_enable); filter_stats_read() returns and clears them."""
    device = torch.device(device)
    with torch.cuda.device(device):
        if on:
            buf = torch.zeros(16, dtype=torch.int64, device=device)
            _FILTER_STATS[device.index] = buf
            _lib.check(_lib.load().am_filter_stats_enable(_ptr(buf)), "am_filter_stats_enable")
        else:
            _FILTER_STATS.pop(device.index, None)
            _lib.check(_lib.load().am_filter_stats_enable(ctypes.c_void_p(None)), "am_filter_stats_enable")


def filter_stats_read(device):
    buf = _FILTER_STATS[torch.device(device).index]
    values = buf.cpu().tolist()
    buf.zero_()
    out = dict(zip(FILTER_STATS_NAMES, values))
    # slot 9 holds the bit pattern of a float: the largest measured |f16 value - exact value| / (fast_c (|x|^2 + G))
    out["bound_ratio_max"] = struct.unpack("<f", struct.pack("<I", int(out["bound_ratio_max"]) & 0xffffffff))[0]
    return out


def _call(lib, name, device, *args):
    """Call entry point `name` with `device` current and torch's current stream of THAT device appended as the
    trailing am_stream_t argument: the library launches on the device that is current in the calling thread, and the
    tensors may live on another one than the thread's (AudioMetrics(device_indices=[1]) while cuda:0 is current)."""
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        args = (*args, ctypes.c_void_p(stream.cuda_stream))
        timer = KernelTimer.active
        if timer is not None:
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record(stream)
            status = getattr(lib, name)(*args)
            b.record(stream)
            timer.records.append((name, a, b))
        else:
            status = getattr(lib, name)(*args)
    _lib.check(status, name)


def _run(name, dev, query, query_args, *args):
    """Entry point `name` with its workspace: the size is what the host query `query` answers for `query_args`, and the
    workspace pointer and that size are the last two C arguments before the stream.  Returns the workspace (the calls that
    leave a flag word at its head read it back)."""
    lib = _lib.load()
    nb = getattr(lib, query)(*query_args)
    ws = _workspace(nb, dev)
    _call(lib, name, dev, *args, _ptr(ws), nb)
    return ws


def _query(stem, f64):
    """The name of the workspace query of the float64 (am_<stem>_f64_workspace_bytes) or float32 form of an entry point."""
    return f"am_{stem}_f64_workspace_bytes" if f64 else f"am_{stem}_workspace_bytes"


_HOST_CAPS = {}


def _host_cap(entry):
    """The answer of a host query without arguments (a compile-time limit of the library), asked once."""
    if entry not in _HOST_CAPS:
        _HOST_CAPS[entry] = int(getattr(_lib.load(), entry)())
    return _HOST_CAPS[entry]


def _require_cuda(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.HipLibraryError(
            f"{name} must be a tensor resident on the MI355X (got {type(t).__name__} on "
            f"{getattr(t, 'device', 'host')}); this package has no CPU fallback")


def _same_device(*tensors):
    dev = tensors[0].device
    for t in tensors[1:]:
        if t.device != dev:
            raise ValueError(f"tensors on different devices: {dev} and {t.device}")
    return dev


def is_f64(t):
    return torch.is_tensor(t) and t.dtype == torch.float64


def as_matrix(e, name="embeddings"):
    """(N, D) f32 device matrix with unit column stride, 16-B aligned rows
    (row stride % 4 == 0).  Copies (zero-padding the row stride) only if needed."""
    _require_cuda(e, name)
    if e.dim() != 2:
        raise ValueError(f"{name} must be 2-D, got shape {tuple(e.shape)}")
    if e.dtype != torch.float32:
        e = e.to(torch.float32)
    n, d = e.shape
    ok = e.stride(1) == 1 and e.stride(0) % 4 == 0 and e.stride(0) >= d and e.data_ptr() % 16 == 0
    if n > 0 and not ok:
        ld = (d + 3) // 4 * 4
        buf = torch.zeros((n, ld), dtype=torch.float32, device=e.device)
        buf[:, :d] = e
        e = buf[:, :d]
    return e


def as_matrix64(e, name="embeddings"):
    """(N, D) f64 device matrix with unit column stride (the f64 kernels need no alignment: any row stride >= D)."""
    _require_cuda(e, name)
    if e.dim() != 2:
        raise ValueError(f"{name} must be 2-D, got shape {tuple(e.shape)}")
    if e.dtype != torch.float64:
        e = e.to(torch.float64)
    n, d = e.shape
    if n > 0 and (e.stride(1) != 1 or (n > 1 and e.stride(0) < d)):
        e = e.contiguous()
    return e


def as_rows(e, name="embeddings"):
    """The matrix form the kernels take, in the dtype the reference computes in (data.py:39-44, prdc.py:12, kd.py:115):
    float64 rows stay float64 (the *_f64 entry points), everything else is float32."""
    return as_matrix64(e, name) if is_f64(e) else as_matrix(e, name)


def _ld64(e):
    return e.stride(0) if e.shape[0] > 1 else e.shape[1]


def _ld(e):
    """Leading dimension handed to the C ABI (a 1-row view may carry any stride)."""
    if e.shape[0] > 1:
        return e.stride(0)
    return (e.shape[1] + 3) // 4 * 4


def _rows(e, name, f64):
    """(the matrix form the float64 / float32 entry points take, its leading dimension, their suffix "f64" / "f32")"""
    if f64:
        e = as_matrix64(e, name)
        return e, _ld64(e), "f64"
    e = as_matrix(e, name)
    return e, _ld(e), "f32"


def _any_f64(*sets):
    """The promotion rule of the reference's numpy code: float64 rows on either side make every set float64."""
    return any(is_f64(t) for t in sets)


def _both_f64(what, *sets):
    """The rule of the Kernel Audio Distance calls: True when every set holds float64 rows (the *_f64 entry points), False
    when none does; a mixed pair is refused before anything touches the tensors."""
    wide = [is_f64(t) for t in sets]
    if any(wide) and not all(wide):
        raise NotImplementedError(f"{what} takes float32 rows, or float64 rows in BOTH sets (a mixed pair is not implemented: "
                                  "convert one side)")
    return all(wide)


def _f64(t, name):
    _require_cuda(t, name)
    if t.dtype != torch.float64 or not t.is_contiguous():
        t = t.to(torch.float64).contiguous()
    return t


# ------------------------------------------------------------------ two sets of float32 rows
def _refuse_f64(op, *tensors):
    if any(is_f64(t) for t in tensors):
        raise NotImplementedError(f"{op} takes float32 rows (the float64 matrix-core form is not implemented)")


def _check_two_sets(op, x, y, both="x and y", sides=True):
    """The shape checks of the row-sweep ops: both sets 2-D (`both` names them), of one width and - sides=False: the op words
    that itself - with rows on both sides."""
    if x.dim() != 2 or y.dim() != 2:
        raise ValueError(f"{both} must be 2-D, got shapes {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"feature widths differ: {x.shape[1]} and {y.shape[1]}")
    if sides and (x.shape[0] < 1 or y.shape[0] < 1 or x.shape[1] < 1):
        raise ValueError(f"{op} needs rows on both sides (got shapes {tuple(x.shape)} and {tuple(y.shape)})")


def _two_sets(x, y, names=("x", "y"), more=()):
    """(x, y, device, n, m, d) of two checked sets in the form the kernels take - prepared once when `x is y` - on one device
    with the (tensor, name) pairs of `more`, the vectors that go with them."""
    same = x is y
    x = as_matrix(x, names[0])
    y = x if same else as_matrix(y, names[1])
    for t, name in more:
        _require_cuda(t, name)
    dev = _same_device(x, y, *(t for t, _ in more))
    return x, y, dev, x.shape[0], y.shape[0], x.shape[1]


def _check_gram_rows(op, x, y, widths=True):
    """The row checks of the float32 Gram ops: no float64 side (named), both 2-D tensors and - widths=True - of one width."""
    for t, name in ((x, "x"), (y, "y")):
        if is_f64(t):
            raise NotImplementedError(f"{op} takes float32 rows ({name} holds float64 rows; the float64 matrix-core "
                                      "form is not implemented)")
        if not torch.is_tensor(t) or t.dim() != 2:
            raise ValueError(f"{name} must be a 2-D tensor, got {tuple(getattr(t, 'shape', ()))}")
    if widths and x.shape[1] != y.shape[1]:
        raise ValueError(f"feature widths differ: {x.shape[1]} and {y.shape[1]}")


def _blocks_mask(blocks):
    blocks = int(blocks)
    if blocks < 1 or blocks > 7:
        raise ValueError(f"blocks={blocks} is not a mask of MMD_XX | MMD_YY | MMD_XY")
    return blocks


# ------------------------------------------------------------------ row groups: rows[idx[offsets[b]:offsets[b + 1]]]
def _group_offsets(offsets):
    """(the offsets as a list of ints, B, the same as a ctypes int64 array for the C ABI)."""
    offs = [int(o) for o in offsets]
    b = len(offs) - 1
    if b < 1 or offs[0] != 0 or any(offs[i + 1] <= offs[i] for i in range(b)):
        raise ValueError(f"offsets must start at 0 and increase strictly (got {offs[:4]}{'...' if b > 3 else ''})")
    return offs, b, (ctypes.c_int64 * (b + 1))(*offs)


def _group_index(idx, listed, like):
    """The index list as a contiguous int64 tensor on the device of `like` with at least `listed` entries; None (the rows
    in stored order, where the entry point allows it) passes through."""
    if idx is None:
        return None
    _require_cuda(idx, "idx")
    idx = idx.to(torch.int64).contiguous()
    _same_device(like, idx)
    if idx.numel() < listed:
        raise ValueError(f"idx holds {idx.numel()} entries, offsets name {listed}")
    return idx


def _index_check(ws, idx, n, noun):
    """check() of a group-list call: the one host read of the flag word at the head of its workspace - 1 + the position
    of an index outside [0, n), or 0.  Without an index list the offending value is the position itself."""
    def check():
        flag = int(ws[:8].view(torch.int64).item())
        if flag != 0:
            pos = flag - 1
            bad = int(idx[pos].item()) if idx is not None else pos
            raise ValueError(f"idx[{pos}] = {bad} is outside [0, {n}) ({noun} are named by stored-row index)")
    return check


def _records_out(out, b, dev, whose):
    """The f64 [B, 5] record tensor of the batched Frechet entry points: a fresh one, or the caller's once checked."""
    if out is None:
        return torch.empty((b, 5), dtype=torch.float64, device=dev)
    if out.dtype != torch.float64 or tuple(out.shape) != (b, 5) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous float64 [B, 5] tensor on the {whose} device")
    return out


def _bandwidth_args(bw2, gamma):
    """The (bw2 pointer, gamma) arguments of the Gaussian-kernel entry points from exactly one of a float32 device scalar
    and a number."""
    if (bw2 is None) == (gamma is None):
        raise ValueError("exactly one of bw2 (device scalar) and gamma (number) must be given")
    if bw2 is None:
        return ctypes.c_void_p(None), float(gamma)
    _require_cuda(bw2, "bw2")
    if bw2.dtype != torch.float32 or bw2.numel() != 1:
        raise ValueError("bw2 must be a float32 device scalar")
    return _ptr(bw2), 0.0


# ------------------------------------------------------------------ statistics
def _stats(e, f64):
    e, ld, kind = _rows(e, "embeddings", f64)
    n, d = e.shape
    mean = torch.empty(d, dtype=torch.float64, device=e.device)
    cov = torch.empty((d, d), dtype=torch.float64, device=e.device)
    _run("am_stats_" + kind, e.device, _query("stats", f64), (n, d), _ptr(e), n, d, ld, _ptr(mean), _ptr(cov))
    return mean, cov


def stats(e):
    """mean f64[D], unbiased covariance f64[D, D] of the rows of e (data.py:37-58), computed in the dtype of e."""
    return stats_f64(e) if is_f64(e) else _stats(e, False)


def stats_f64(e):
    """mean f64[D], unbiased covariance f64[D, D] of the rows of a FLOAT64 device matrix, every step in f64 (am_stats_f64):
    the reference computes in the dtype it is given (data.py:39-44)."""
    _require_cuda(e, "embeddings")
    if e.dim() != 2 or e.dtype != torch.float64:
        raise ValueError(f"stats_f64 takes a 2-D float64 matrix, got {tuple(e.shape)} {e.dtype}")
    return _stats(e, True)


def stats_gather(x, idx, offsets, defer_check=False):
    """Statistics of B index-gathered subsets of the stored matrix x in one library call (am_stats_gather_f32 / _f64, by
    the dtype of x): subset b is the rows x[idx[offsets[b]:offsets[b + 1]]].  idx: int64 device tensor, offsets: B + 1
    host integers starting at 0.  Returns (means f64 [B, D], covs f64 [B, D, D]).  An index outside [0, N) raises
    ValueError - the kernels never dereference it, they leave its position in the workspace's flag word.
    defer_check=True returns (means, covs, check) without waiting for the device; the caller runs check() - the one host
    read of the flag word - once it has queued the work that consumes the statistics."""
    x, ld, kind = _rows(x, "embeddings", is_f64(x))
    _require_cuda(idx, "idx")
    n, d = x.shape
    offs, b, host_offs = _group_offsets(offsets)
    idx = _group_index(idx, offs[-1], x)
    dev = x.device
    means = torch.empty((b, d), dtype=torch.float64, device=dev)
    covs = torch.empty((b, d, d), dtype=torch.float64, device=dev)
    ws = _run("am_stats_gather_" + kind, dev, "am_stats_gather_workspace_bytes", (offs[-1], b, d), _ptr(x), n, ld, d, _ptr(idx),
              _host(host_offs), b, _ptr(means), _ptr(covs))
    check = _index_check(ws, idx, n, "subset rows")
    if defer_check:
        return means, covs, check
    check()
    return means, covs


def colsum(e):
    f64 = is_f64(e)
    e, ld, kind = _rows(e, "embeddings", f64)
    n, d = e.shape
    out = torch.empty(d, dtype=torch.float64, device=e.device)
    _run("am_colsum_" + kind, e.device, _query("stats", f64), (n, d), _ptr(e), n, d, ld, _ptr(out))
    return out


def scatter(e, mean):
    """sum_n (x_n - mean)(x_n - mean)^T, not divided (multi-GPU building block)."""
    mean = _f64(mean, "mean")
    f64 = is_f64(e)
    e, ld, kind = _rows(e, "embeddings", f64)
    n, d = e.shape
    out = torch.empty((d, d), dtype=torch.float64, device=e.device)
    _run("am_scatter_" + kind, e.device, _query("stats", f64), (n, d), _ptr(e), n, d, ld, _ptr(mean), _ptr(out))
    return out


def stats_merge(n1, mean1, cov1, n2, mean2, cov2, inplace=False):
    """Chan merge (data.py:77-94).  inplace=True overwrites (mean1, cov1)."""
    lib = _lib.load()
    mean1, cov1, mean2, cov2 = (_f64(t, "stats") for t in (mean1, cov1, mean2, cov2))
    d = mean1.numel()
    # the C ABI sees raw pointers: a (1, 1) covariance (recompute_stats' n == 1 quirk) would be read and written as D x D
    if mean2.numel() != d or tuple(cov1.shape) != (d, d) or tuple(cov2.shape) != (d, d):
        raise ValueError(f"stats_merge: inconsistent shapes mean {tuple(mean1.shape)}/{tuple(mean2.shape)}, "
                         f"cov {tuple(cov1.shape)}/{tuple(cov2.shape)}")
    _same_device(mean1, cov1, mean2, cov2)
    om = mean1 if inplace else torch.empty_like(mean1)
    oc = cov1 if inplace else torch.empty_like(cov1)
    _call(lib, "am_stats_merge_f64", mean1.device, int(n1), _ptr(mean1), _ptr(cov1), int(n2), _ptr(mean2), _ptr(cov2), d,
                                      _ptr(om), _ptr(oc))
    return om, oc


def stats_push_max_rows():
    return _host_cap("am_stats_push_max_rows")


def stats_push(e, n_old, mean_in, mean_out, cov, rows_out=None, ld_out=0):
    """One launch for AudioMetricsData.add(batch) of a small batch (am_stats_push_f32; data.py:37-47, 68-72, 77-94): batch
    statistics, Chan merge into (n_old, mean_in, cov) -> (mean_out, cov in place), rows copied to `rows_out` (the row
    n_old of the store, row stride ld_out) when given.  The caller owns every buffer; nothing is allocated here - this is
    the per-batch hot path of the embedding pipeline, so the glue is kept to one ctypes call."""
    lib = _lib.load()
    dev = e.device
    with torch.cuda.device(dev):
        status = lib.am_stats_push_f32(e.data_ptr(), e.shape[0], e.shape[1], e.stride(0) if e.shape[0] > 1 else e.shape[1],
                                       int(n_old), mean_in.data_ptr() if mean_in is not None else None, mean_out.data_ptr(),
                                       cov.data_ptr(), rows_out.data_ptr() if rows_out is not None else None, int(ld_out),
                                       torch.cuda.current_stream(dev).cuda_stream)
    if status != 0:
        _lib.check(status, "am_stats_push_f32")


# ------------------------------------------------------------------ PCA projection support
def eigh_descending(a, max_sweeps=40):
    """(eigenvalues f64[D] descending, eigenvectors f64[D, D] with row i = vector i) of a symmetric PSD matrix."""
    a = _f64(a, "matrix")
    d = a.shape[0]
    if a.dim() != 2 or a.shape[1] != d:
        raise ValueError(f"expected a square matrix, got {tuple(a.shape)}")
    evals = torch.empty(d, dtype=torch.float64, device=a.device)
    evecs = torch.empty((d, d), dtype=torch.float64, device=a.device)
    _run("am_eigh_sym_f64", a.device, "am_eigh_workspace_bytes", (d,), _ptr(a), d, _ptr(evals), _ptr(evecs), int(max_sweeps))
    return evals, evecs


def project(x, mean, components):
    """(x - mean) @ components.T as f64 [N, p] (IncrementalPCA.transform)."""
    lib = _lib.load()
    x, ld, kind = _rows(x, "embeddings", is_f64(x))
    mean, components = _f64(mean, "mean"), _f64(components, "components")
    n, d = x.shape
    p = components.shape[0]
    if mean.numel() != d or components.dim() != 2 or components.shape[1] != d:
        raise ValueError(f"projection shapes do not match: x {tuple(x.shape)}, mean {tuple(mean.shape)}, components {tuple(components.shape)}")
    _same_device(x, mean, components)
    out = torch.empty((n, p), dtype=torch.float64, device=x.device)
    if n > 0:
        _call(lib, "am_project_rows_f64" if kind == "f64" else "am_project_f64", x.device, _ptr(x), n, ld, d, _ptr(mean),
              _ptr(components), p, _ptr(out))
    return out


# ------------------------------------------------------------------ Frechet
def _frechet_stats(mu_x, cov_x, mu_y, cov_y):
    """The statistics of frechet / frechet_maps as contiguous f64 device tensors of one D, then D and their device."""
    mu_x, cov_x, mu_y, cov_y = (_f64(t, "stats") for t in (mu_x, cov_x, mu_y, cov_y))
    d = mu_x.numel()
    if cov_x.shape != (d, d) or cov_y.shape != (d, d) or mu_y.numel() != d:
        raise ValueError(f"inconsistent shapes: mu {tuple(mu_x.shape)}/{tuple(mu_y.shape)}, "
                         f"cov {tuple(cov_x.shape)}/{tuple(cov_y.shape)}")
    return mu_x, cov_x, mu_y, cov_y, d, _same_device(mu_x, cov_x, mu_y, cov_y)


def frechet(mu_x, cov_x, mu_y, cov_y, max_iter=64, tol=1e-13):
    mu_x, cov_x, mu_y, cov_y, d, dev = _frechet_stats(mu_x, cov_x, mu_y, cov_y)
    out = (ctypes.c_double * 4)()
    _run("am_frechet_f64", dev, "am_frechet_workspace_bytes", (d,), _ptr(mu_x), _ptr(cov_x), _ptr(mu_y), _ptr(cov_y), d,
         int(max_iter), float(tol), _host(out))
    return dict(fd=out[0], tr_sqrt=out[1], iters=int(out[2]), resid=out[3])


def frechet_maps(mu_x, cov_x, mu_y, cov_y, max_iter=64, tol=1e-13):
    """frechet() plus the Gaussian optimal-transport maps (am_frechet_maps_f64): the dict of frechet() - the same bits -
    with "stop" (the solver's stop code; 1 = converged), "map_xy" (the symmetric A with A cov_x A = cov_y) and "map_yx" (its
    inverse), both f64 device [D, D], exactly symmetric, and all NaN unless stop == 1."""
    mu_x, cov_x, mu_y, cov_y, d, dev = _frechet_stats(mu_x, cov_x, mu_y, cov_y)
    out = (ctypes.c_double * 5)()
    map_xy = torch.empty((d, d), dtype=torch.float64, device=dev)
    map_yx = torch.empty((d, d), dtype=torch.float64, device=dev)
    _run("am_frechet_maps_f64", dev, "am_frechet_maps_workspace_bytes", (d,), _ptr(mu_x), _ptr(cov_x), _ptr(mu_y), _ptr(cov_y), d,
         int(max_iter), float(tol), _host(out), _ptr(map_xy), _ptr(map_yx))
    return dict(fd=out[0], tr_sqrt=out[1], iters=int(out[2]), resid=out[3], stop=int(out[4]), map_xy=map_xy, map_yx=map_yx)


def frechet_influence(rows, mu, b, lin, c0):
    """psi_i = c_i^T b c_i + lin^T c_i + c0 with c_i = rows_i - mu (am_frechet_influence_f32 / _f64, by the dtype of rows;
    all arithmetic in f64, the same bits for float32 rows and their float64 copies).  mu, lin: f64 device [D]; b: f64 device
    [D, D], symmetric; c0: a number.  Returns (psi f64 [N], sums f64 [4] = {sum psi, sum psi^2, finite rows, non-finite
    rows}), both on the device; a row with a non-finite element has psi = NaN and is left out of the sums."""
    rows, ld, kind = _rows(rows, "rows", is_f64(rows))
    n, d = rows.shape
    mu, b, lin = (_f64(t, "influence terms") for t in (mu, b, lin))
    if n < 1 or mu.numel() != d or lin.numel() != d or tuple(b.shape) != (d, d):
        raise ValueError(f"inconsistent shapes: rows {tuple(rows.shape)}, mu {tuple(mu.shape)}, b {tuple(b.shape)}, lin {tuple(lin.shape)}")
    dev = _same_device(rows, mu, b, lin)
    psi = torch.empty(n, dtype=torch.float64, device=dev)
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    _run("am_frechet_influence_" + kind, dev, "am_frechet_influence_workspace_bytes", (n,), _ptr(rows), n, ld, d, _ptr(mu), _ptr(b),
         _ptr(lin), float(c0), _ptr(psi), _ptr(sums))
    return psi, sums


LOGIT_MAX_MODELS = 16


def logit_pass(rows, fold, label, coef, want_z=True):
    """One fused pass of K linear logistic probes over the rows of ONE class (am_logit_pass_f32 / _f64, by the dtype of rows;
    all arithmetic in f64, the same bits for float32 rows and their float64 copies).  fold: int32 device [N] (-1: the row
    takes no part, 0..K-1: held out of that model, K: trains every model); label: 1 or 0, the class of every row; coef:
    f64 device [K, D + 1], the weights in ROW coordinates and then the intercept.  Returns (sums f64 [K, D + 2] = {sum r x,
    sum r, sum loss} over each model's training rows, z f64 [N] - the logit of every row under the model of its own fold,
    NaN where it has none - or None with want_z=False, counts f64 [2] = {rows that took part, rows with a non-finite
    element}), all on the device, stream-ordered, nothing waits for the device.  Two calls return the same bits."""
    rows, ld, kind = _rows(rows, "rows", is_f64(rows))
    n, d = rows.shape
    coef = _f64(coef, "coef")
    _require_cuda(fold, "fold")
    if label not in (0, 1):
        raise ValueError(f"label={label!r} must be 1 or 0 (the class of every row)")
    if coef.dim() != 2 or coef.shape[1] != d + 1 or not 1 <= coef.shape[0] <= LOGIT_MAX_MODELS:
        raise ValueError(f"coef must be [K, D + 1] with 1 <= K <= {LOGIT_MAX_MODELS} and D = {d}, got shape {tuple(coef.shape)}")
    if n < 1 or fold.dim() != 1 or fold.shape[0] != n or fold.dtype != torch.int32:
        raise ValueError(f"fold must be an int32 tensor with one entry per row ({n}), got {fold.dtype} {tuple(fold.shape)}")
    fold = fold.contiguous()
    dev = _same_device(rows, fold, coef)
    k = coef.shape[0]
    sums = torch.empty((k, d + 2), dtype=torch.float64, device=dev)
    z = torch.empty(n, dtype=torch.float64, device=dev) if want_z else None
    counts = torch.empty(2, dtype=torch.float64, device=dev)
    _run("am_logit_pass_" + kind, dev, "am_logit_pass_workspace_bytes", (n, d, k), _ptr(rows), n, ld, d, _ptr(fold), int(label),
         _ptr(coef), k, _ptr(sums), _opt(z), _ptr(counts))
    return sums, z, counts


FRECHET_BATCH_WS_CAP = 1 << 30     # bytes of solver workspace per library call; larger batches go in chunks of sets


def frechet_batch(mu_x, cov_x, mu_y, cov_y, max_iter=64, tol=1e-13, out=None):
    """B Frechet distances advancing together (am_frechet_batch_f64): mu_x [B, D], cov_x [B, D, D] against mu_y [D],
    cov_y [D, D] (one reference shared by all sets) or mu_y [B, D], cov_y [B, D, D].  Returns the list of the per-set dicts
    frechet() returns, plus the device-side stop code under "stop".  `out` (optional, f64 device [B, 5]) receives the raw
    records; it is written for every set even when a set with a non-finite product makes the call raise HipLibraryError."""
    lib = _lib.load()
    mu_x, cov_x, mu_y, cov_y = (_f64(t, "stats") for t in (mu_x, cov_x, mu_y, cov_y))
    if mu_x.dim() != 2 or cov_x.dim() != 3:
        raise ValueError(f"mu_x must be [B, D] and cov_x [B, D, D], got {tuple(mu_x.shape)} and {tuple(cov_x.shape)}")
    b, d = mu_x.shape
    shared = mu_y.dim() == 1
    want_y = ((d,), (d, d)) if shared else ((b, d), (b, d, d))
    if b < 1 or tuple(cov_x.shape) != (b, d, d) or (tuple(mu_y.shape), tuple(cov_y.shape)) != want_y:
        raise ValueError(f"inconsistent shapes: mu {tuple(mu_x.shape)}/{tuple(mu_y.shape)}, "
                         f"cov {tuple(cov_x.shape)}/{tuple(cov_y.shape)}")
    dev = _same_device(mu_x, cov_x, mu_y, cov_y)
    out = _records_out(out, b, dev, "statistics'")
    per_set = max(int(lib.am_frechet_batch_workspace_bytes(1, d)), 1)
    chunk = max(1, min(b, FRECHET_BATCH_WS_CAP // per_set))
    failure = None
    for s0 in range(0, b, chunk):
        s1 = min(b, s0 + chunk)
        try:
            _run("am_frechet_batch_f64", dev, "am_frechet_batch_workspace_bytes", (s1 - s0, d), _ptr(mu_x[s0:s1]), _ptr(cov_x[s0:s1]),
                 _ptr(mu_y if shared else mu_y[s0:s1]), _ptr(cov_y if shared else cov_y[s0:s1]), 0 if shared else 1, s1 - s0, d,
                 int(max_iter), float(tol), _ptr(out[s0:s1]))
        except _lib.HipLibraryError as e:                     # (a stop code 4 in this chunk; the other chunks still run)
            failure = failure or e
    rec = out.cpu().tolist()                                  # one device -> host copy of B x 5 doubles
    bad = [i for i, r in enumerate(rec) if int(r[4]) == 4]
    if bad:
        raise _lib.HipLibraryError(f"am_frechet_batch_f64: set {bad[0]} of {b}: non-finite covariance product or trace in "
                                   f"Newton-Schulz (sets with stop code 4: {bad})") from failure
    if failure is not None:
        raise failure
    return [dict(fd=r[0], tr_sqrt=r[1], iters=int(r[2]), resid=r[3], stop=int(r[4])) for r in rec]


def frechet_groups_max_rows():
    return _host_cap("am_frechet_groups_max_rows")


def frechet_groups(rows, idx, offsets, mu_y, cov_y, out=None):
    """Per-group Frechet distances in the dual form (am_frechet_groups_f32 / _f64, by the dtype of rows): group b is the
    rows rows[idx[offsets[b]:offsets[b + 1]]] (idx: int64 device tensor, or None for the rows in stored order; offsets:
    B + 1 host integers starting at 0), every group of 1 .. frechet_groups_max_rows() rows, scored against the one
    reference (mu_y [D], cov_y [D, D]).  Nothing waits for the device: returns (out, check) with out the f64 device tensor
    [B, 5] of { fd, tr_sqrt, sweeps, residual, stop code } records and check() the one host read of the workspace's flag
    word, which raises ValueError for an index outside [0, N) (the kernels never dereference it)."""
    rows, ld, kind = _rows(rows, "embeddings", is_f64(rows))
    n, d = rows.shape
    mu_y, cov_y = _f64(mu_y, "mu_y"), _f64(cov_y, "cov_y")
    if mu_y.numel() != d or tuple(cov_y.shape) != (d, d):
        raise ValueError(f"inconsistent shapes: rows {tuple(rows.shape)}, mu_y {tuple(mu_y.shape)}, cov_y {tuple(cov_y.shape)}")
    offs, b, host_offs = _group_offsets(offsets)
    dev = _same_device(rows, mu_y, cov_y)
    idx = _group_index(idx, offs[-1], rows)
    out = _records_out(out, b, dev, "rows'")
    ws = _run("am_frechet_groups_" + kind, dev, "am_frechet_groups_workspace_bytes", (offs[-1], b, d), _ptr(rows), n, ld, d, _opt(idx),
              _host(host_offs), b, _ptr(mu_y), _ptr(cov_y), _ptr(out))
    return out, _index_check(ws, idx, n, "group rows")


# ------------------------------------------------------------------ Vendi score
VENDI_KERNELS = {"cosine": 0, "gaussian": 1}                 # enum am_vendi_kernel


def vendi_groups_max_rows():
    return _host_cap("am_vendi_groups_max_rows")


def vendi_gram_max_rows():
    return _host_cap("am_vendi_gram_max_rows")


def _vendi_kernel_args(kernel, gamma, gamma_dev):
    """(kernel code, gamma, gamma_dev pointer) of the am_vendi_* entry points; no device call.  The cosine kernel takes no
    width; the Gaussian one exactly one of a number and a float32 device scalar holding a median squared distance."""
    if kernel not in VENDI_KERNELS:
        raise ValueError(f"kernel={kernel!r} must be one of {sorted(VENDI_KERNELS)}")
    if kernel == "cosine":
        if gamma is not None or gamma_dev is not None:
            raise ValueError("the cosine kernel takes neither gamma nor gamma_dev")
        return 0, 0.0, ctypes.c_void_p(None)
    dev_arg, gamma_arg = _bandwidth_args(gamma_dev, gamma)
    if gamma_dev is None and not (gamma_arg > 0.0 and gamma_arg < float("inf")):
        raise ValueError(f"gamma={gamma!r} must be a finite positive number")
    return 1, gamma_arg, dev_arg


def _whole_set_check(ws, idx, n, noun):
    """check() of am_vendi_gram_* / am_vendi_moment_*: the one host read of the two flag words at the head of the
    workspace.  An index outside [0, n) raises ValueError; a row without a similarity (zero norm, or a non-finite element)
    is returned as its position, None when every row has one."""
    def check():
        flags = ws[:16].view(torch.int64).cpu().tolist()
        if flags[0] != 0:
            pos = flags[0] - 1
            bad = int(idx[pos].item()) if idx is not None else pos
            raise ValueError(f"idx[{pos}] = {bad} is outside [0, {n}) ({noun} are named by stored-row index)")
        return flags[1] - 1 if flags[1] != 0 else None
    return check


def vendi_groups(rows, idx, offsets, kernel="cosine", gamma=None, gamma_dev=None):
    """The eigenvalues of K / n and the order-1 Vendi score of every group of rows (am_vendi_groups_f32 / _f64, by the dtype
    of rows; the group list as frechet_groups takes it), every group of 1 .. vendi_groups_max_rows() rows.  kernel:
    "cosine", or "gaussian" with exactly one of gamma (a number) and gamma_dev (a float32 device scalar holding a median
    squared distance: gamma = 0.5 / it, formed on the device).  Nothing waits for the device: returns (rec, evals, check)
    with rec the f64 device tensor [B, 8] of { vendi, entropy, rank, lambda_max, sweeps, residual, stop code, 0 } records,
    evals the f64 device tensor [n_total] of each group's eigenvalues at its list positions (descending, those at or below
    4 n 2^-52 lambda_max as 0), and check() the one host read of the workspace's flag word, which raises ValueError for an
    index outside [0, N)."""
    code, gamma_arg, dev_arg = _vendi_kernel_args(kernel, gamma, gamma_dev)
    offs, b, host_offs = _group_offsets(offsets)
    rows, ld, kind = _rows(rows, "embeddings", is_f64(rows))
    n, d = rows.shape
    dev = rows.device
    if gamma_dev is not None:
        _same_device(rows, gamma_dev)
    idx = _group_index(idx, offs[-1], rows)
    rec = torch.empty((b, 8), dtype=torch.float64, device=dev)
    evals = torch.empty(offs[-1], dtype=torch.float64, device=dev)
    ws = _run("am_vendi_groups_" + kind, dev, "am_vendi_groups_workspace_bytes", (offs[-1], b, d), _ptr(rows), n, ld, d, _opt(idx),
              _host(host_offs), b, code, gamma_arg, dev_arg, _ptr(rec), _ptr(evals))
    return rec, evals, _index_check(ws, idx, n, "group rows")


def vendi_gram(rows, idx=None, kernel="cosine", gamma=None, gamma_dev=None):
    """M = K / n of the rows rows[idx] (idx None: all rows) as an f64 device tensor [n, n] (am_vendi_gram_f32 / _f64):
    exactly symmetric, diagonal exactly 1 / n, n <= vendi_gram_max_rows().  Returns (m, check); nothing waits for the
    device.  check() raises ValueError for an index outside [0, N) and returns the position of a row without a similarity
    (zero norm under the cosine kernel, or a non-finite element; such a row counts as zeros in m), or None."""
    code, gamma_arg, dev_arg = _vendi_kernel_args(kernel, gamma, gamma_dev)
    n_rows = int(rows.shape[0]) if idx is None else int(idx.numel())
    if not 1 <= n_rows <= vendi_gram_max_rows():
        raise ValueError(f"vendi_gram takes 1 .. {vendi_gram_max_rows()} rows, got {n_rows}")
    rows, ld, kind = _rows(rows, "embeddings", is_f64(rows))
    n, d = rows.shape
    dev = rows.device
    if gamma_dev is not None:
        _same_device(rows, gamma_dev)
    idx = _group_index(idx, n_rows, rows)
    m = torch.empty((n_rows, n_rows), dtype=torch.float64, device=dev)
    ws = _run("am_vendi_gram_" + kind, dev, "am_vendi_gram_workspace_bytes", (n_rows, d), _ptr(rows), n, ld, d, _opt(idx), n_rows, code,
              gamma_arg, dev_arg, _ptr(m))
    return m, _whole_set_check(ws, idx, n, "rows")


def vendi_moment_chunks(n, d):
    """The number of row chunks am_vendi_moment_* folds for n rows of d columns (a host query)."""
    return int(_lib.load().am_vendi_moment_chunks(int(n), int(d)))


def vendi_moment(rows):
    """S = (1 / n) sum_i x_i x_i^T / |x_i|^2 over all rows as an f64 device tensor [D, D] (am_vendi_moment_f32 / _f64): the
    dual form of the cosine kernel's K / n, with the same non-zero eigenvalues.  Returns (s, check) as vendi_gram does."""
    if rows.dim() != 2 or rows.shape[0] < 1:
        raise ValueError(f"vendi_moment takes a non-empty 2-D matrix of rows, got shape {tuple(rows.shape)}")
    rows, ld, kind = _rows(rows, "embeddings", is_f64(rows))
    n, d = rows.shape
    s = torch.empty((d, d), dtype=torch.float64, device=rows.device)
    ws = _run("am_vendi_moment_" + kind, rows.device, "am_vendi_moment_workspace_bytes", (n, d), _ptr(rows), n, ld, d, _ptr(s))
    return s, _whole_set_check(ws, None, n, "rows")


class FrechetJob:
    """A Frechet solve in flight on a side stream (frechet_async).  Nothing here blocks the host until .result()."""

    def __init__(self, stats, max_iter, tol):
        lib = _lib.load()
        self._stats = stats                                  # keeps the operands alive
        self._max_iter, self._tol = int(max_iter), float(tol)
        dev = stats[0].device
        self._d = stats[0].numel()
        self._nb = lib.am_frechet_workspace_bytes(self._d)
        main = torch.cuda.current_stream(dev)
        self._side = _side_stream(("fad", dev.index), dev)
        self._side.wait_stream(main)                         # the statistics were produced on the caller's stream
        with torch.cuda.stream(self._side):
            self._ws = _workspace(self._nb, dev)
            self._out = torch.empty(8, dtype=torch.float64, device=dev)
            self._next = 0
            self._enqueue(lib.am_frechet_first_block())
        for t in stats:
            t.record_stream(self._side)

    def _enqueue(self, n_iter):
        lib = _lib.load()
        mu_x, cov_x, mu_y, cov_y = self._stats
        n_iter = min(int(n_iter), self._max_iter - self._next)
        with torch.cuda.stream(self._side):
            _call(lib, "am_frechet_enqueue_f64", mu_x.device, _ptr(mu_x), _ptr(cov_x), _ptr(mu_y), _ptr(cov_y), self._d,
                  self._next, n_iter, self._max_iter, self._tol, _ptr(self._out), _ptr(self._ws), self._nb)
        self._next += n_iter

    def result(self):
        lib = _lib.load()
        while True:
            with torch.cuda.stream(self._side):
                out = self._out.cpu().tolist()               # the one host read (synchronises the side stream only)
            if int(out[4]) != 0 or self._next >= self._max_iter:
                break
            self._enqueue(lib.am_frechet_first_block())      # ill-conditioned product: another block of iterations
        torch.cuda.current_stream(self._stats[0].device).wait_stream(self._side)
        if int(out[4]) == 4:
            raise _lib.HipLibraryError("am_frechet_enqueue_f64: non-finite covariance product or trace in Newton-Schulz")
        return dict(fd=out[0], tr_sqrt=out[1], iters=int(out[2]), resid=out[3])


def frechet_async(mu_x, cov_x, mu_y, cov_y, max_iter=64, tol=1e-13):
    """frechet() enqueued on a side stream behind the work already queued on the current one; the kernels that the
    caller launches next on its own stream overlap it.  The solver decides convergence on the device, so no helper thread
    and no host polling are involved: .result() reads five doubles."""
    stats = tuple(_f64(t, "stats") for t in (mu_x, cov_x, mu_y, cov_y))
    d = stats[0].numel()
    if stats[1].shape != (d, d) or stats[3].shape != (d, d) or stats[2].numel() != d:
        raise ValueError("inconsistent shapes of the statistics")
    _same_device(*stats)
    return FrechetJob(stats, max_iter, tol)


def apa_scalar(d_y_x, d_y_xp, d_x_xp):
    return _lib.load().am_apa_f64(float(d_y_x), float(d_y_xp), float(d_x_xp))


# ------------------------------------------------------------------ kernel distance
def kd_poly(x, y, idx1, idx2, gamma, coef0, degree):
    """Per-subset unbiased MMD^2 (f64[S] device tensor).  idx1/idx2: int64 [S, m].  float64 features (either side: numpy's
    matmul promotes, kd.py:115) run every product and sum in f64 (am_kd_poly_f64)."""
    idx1, idx2 = _index_table(idx1, "idx1"), _index_table(idx2, "idx2")
    s, m = idx1.shape
    f64 = _any_f64(x, y)
    (x, ldx, kind), (y, ldy, _) = _rows(x, "features_1", f64), _rows(y, "features_2", f64)
    d = x.shape[1]
    out = torch.empty(s, dtype=torch.float64, device=x.device)
    query = ("am_kd_f64_workspace_bytes", (s, m)) if f64 else ("am_kd_poly_workspace_bytes", (s, m, d))
    _run("am_kd_poly_" + kind, x.device, *query, _ptr(x), x.shape[0], ldx, _ptr(y), y.shape[0], ldy, d, _ptr(idx1), _ptr(idx2), s, m,
         float(gamma), float(coef0), int(degree), _ptr(out))
    return out


def kd_rbf(x, y, idx1, idx2, sigma):
    """Per-subset unbiased MMD^2 with the RBF kernel exp(-|x-y|^2 / (2 sigma^2)) (f64[S] device tensor)."""
    idx1, idx2 = _index_table(idx1, "idx1"), _index_table(idx2, "idx2")
    s, m = idx1.shape
    f64 = _any_f64(x, y)
    (x, ldx, kind), (y, ldy, _) = _rows(x, "features_1", f64), _rows(y, "features_2", f64)
    out = torch.empty(s, dtype=torch.float64, device=x.device)
    _run("am_kd_rbf_" + kind, x.device, "am_kd_f64_workspace_bytes" if f64 else "am_kd_rbf_workspace_bytes", (s, m), _ptr(x),
         x.shape[0], ldx, _ptr(y), y.shape[0], ldy, x.shape[1], _ptr(idx1), _ptr(idx2), s, m, float(sigma), _ptr(out))
    return out


# ------------------------------------------------------------------ kernel audio distance
MMD_XX, MMD_YY, MMD_XY = 1, 2, 4                       # enum am_mmd_block


def pairwise_select_sq(x, rank=None):
    """The element of 0-based `rank` (None: the lower median, torch.median's convention) among the float32 squared
    distances of the N (N - 1) / 2 unordered row pairs of x, as a 0-dim float32 DEVICE tensor: an exact radix select over
    recomputed Gram tiles (am_pairwise_select_f32; float64 rows: am_pairwise_select_f64, every distance in f64 and the
    result its float32 rounding), stream-ordered, no host synchronisation."""
    f64 = _both_f64("pairwise_select_sq", x)
    x, ld, kind = _rows(x, "x", f64)
    n, d = x.shape
    out = torch.empty((), dtype=torch.float32, device=x.device)
    _run("am_pairwise_select_" + kind, x.device, _query("pairwise_select", f64), (n, d), _ptr(x), n, ld, d,
         -1 if rank is None else int(rank), _ptr(out))
    return out


def mmd_rbf_sums(x, y, bw2=None, gamma=None, blocks=7, out=None):
    """float64[3] device tensor {Sxx, Syy, Sxy} of K = exp(-|a - b|^2 gamma) over the whole sets (am_mmd_rbf_f32; both sets
    float64: am_mmd_rbf_f64): Sxx / Syy over ordered pairs i != j, Sxy over all pairs.  `bw2`: a float32 DEVICE scalar
    (gamma = 0.5 / bw2 is formed on the device - the output of pairwise_select_sq, no host round trip) or `gamma`: a number.
    Only the slots named by `blocks` (MMD_XX | MMD_YY | MMD_XY) are written; the others keep what `out` held (NaN in a
    fresh tensor)."""
    f64 = _both_f64("mmd_rbf_sums", x, y)
    bw2_arg, gamma_arg = _bandwidth_args(bw2, gamma)
    (x, ldx, kind), (y, ldy, _) = _rows(x, "x", f64), _rows(y, "y", f64)
    dev = _same_device(x, y)
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"feature widths differ: {x.shape[1]} and {y.shape[1]}")
    if out is None:
        out = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float64 and out.numel() == 3 and out.is_contiguous()):
        raise ValueError("out must be a contiguous float64[3] device tensor")
    blocks = int(blocks)
    _run("am_mmd_rbf_" + kind, dev, _query("mmd_rbf", f64), (x.shape[0], y.shape[0], x.shape[1], blocks), _ptr(x), x.shape[0], ldx,
         _ptr(y), y.shape[0], ldy, x.shape[1], bw2_arg, gamma_arg, blocks, _ptr(out))
    return out


def mmd_rbf_row_sums(x, y, bw2=None, gamma=None, blocks=7):
    """Two-sided row sums of the Gaussian kernel blocks in one library call (am_mmd_rbf_rows_f32): (out_x, out_y), float64
    device tensors [n, 2] = {w_i, c_i} and [m, 2] = {v_j, r_j} with w_i = sum_{j != i} k(x_i, x_j) (MMD_XX), v_j the same
    inside y (MMD_YY), c_i = sum_j k(x_i, y_j) and r_j = sum_i k(x_i, y_j) (MMD_XY) - every Gram tile computed once, the
    work of mmd_rbf_sums with the same `blocks`.  A side no named block writes is None; a column of a block that is not
    named holds NaN.  `bw2` / `gamma` as for mmd_rbf_sums.  float32 rows only; stream-ordered, nothing waits for the
    device."""
    _check_gram_rows("mmd_rbf_row_sums", x, y)
    blocks = _blocks_mask(blocks)
    bw2_arg, gamma_arg = _bandwidth_args(bw2, gamma)
    x, y = as_matrix(x, "x"), as_matrix(y, "y")
    dev = _same_device(x, y)
    (n, d), m = x.shape, y.shape[0]
    nan = float("nan")
    out_x = torch.full((n, 2), nan, dtype=torch.float64, device=dev) if blocks & (MMD_XX | MMD_XY) else None
    out_y = torch.full((m, 2), nan, dtype=torch.float64, device=dev) if blocks & (MMD_YY | MMD_XY) else None
    _run("am_mmd_rbf_rows_f32", dev, "am_mmd_rbf_rows_workspace_bytes", (n, m, d, blocks), _ptr(x), n, _ld(x), _ptr(y), m, _ld(y), d,
         bw2_arg, gamma_arg, blocks, _opt(out_x), _opt(out_y))
    return out_x, out_y


MMD_CELL = 32                                                        # AM_MMD_CELL: positions per cell


def _cell_units(units, n_pos, name):
    """(U, the ctypes int64 array of the U + 1 cell offsets or None) of one side of mmd_rbf_cell_sums"""
    cells = (n_pos + MMD_CELL - 1) // MMD_CELL
    if units is None:
        return cells, None
    offs = [int(o) for o in units]
    u = len(offs) - 1
    if u < 1 or offs[0] != 0 or offs[-1] != cells or any(offs[i + 1] <= offs[i] for i in range(u)):
        raise ValueError(f"{name} must be cell offsets that start at 0, increase strictly and end at {cells} "
                         f"(got {offs[:4]}{'...' if u > 3 else ''} ending at {offs[-1] if offs else None})")
    return u, (ctypes.c_int64 * (u + 1))(*offs)


def mmd_rbf_cell_sums(x, y, idx_x=None, idx_y=None, units_x=None, units_y=None, blocks=7, gamma=None, bw2=None):
    """Unit-pair sums of the Gaussian kernel blocks in one library call (am_mmd_rbf_cells_f32): (xx [U1, U1], yy [U2, U2],
    xy [U1, U2]), float64 device tensors, None for a block `blocks` (MMD_XX | MMD_YY | MMD_XY) does not name.  A set is a
    list of positions - idx_x / idx_y: int64 device tensors of stored-row indices, -1 for an empty (padding) position; None:
    the rows in stored order.  Cell a is the positions [32 a, 32 a + 32); units_x / units_y: host cell offsets (from 0 to the
    number of cells, strictly increasing), None: every cell is a unit.  Entry [u, v] is the sum of k over the position pairs
    of the two units, inside one set without p == q (by position).  `bw2` / `gamma` as for mmd_rbf_sums.  float32 rows only.
    Where an index list was given the flag word of the call is read back (the one host synchronisation) and an index
    outside [0, n) other than -1 raises ValueError; the kernels never dereference it."""
    _check_gram_rows("mmd_rbf_cell_sums", x, y)
    blocks = _blocks_mask(blocks)
    bw2_arg, gamma_arg = _bandwidth_args(bw2, gamma)
    pos = []
    for idx, rows, name in ((idx_x, x.shape[0], "idx_x"), (idx_y, y.shape[0], "idx_y")):
        if idx is not None and (not torch.is_tensor(idx) or idx.dim() != 1 or idx.numel() == 0 or idx.is_floating_point()):
            raise ValueError(f"{name} must be a non-empty 1-D integer tensor of stored-row indices")
        pos.append(int(idx.numel()) if idx is not None else int(rows))
    (u1, host_ux), (u2, host_uy) = _cell_units(units_x, pos[0], "units_x"), _cell_units(units_y, pos[1], "units_y")
    x, y = as_matrix(x, "x"), as_matrix(y, "y")
    dev = _same_device(x, y)
    idx_x, idx_y = _group_index(idx_x, pos[0], x), _group_index(idx_y, pos[1], y)
    (n, d), m = x.shape, y.shape[0]
    nan = float("nan")
    xx = torch.full((u1, u1), nan, dtype=torch.float64, device=dev) if blocks & MMD_XX else None
    yy = torch.full((u2, u2), nan, dtype=torch.float64, device=dev) if blocks & MMD_YY else None
    xy = torch.full((u1, u2), nan, dtype=torch.float64, device=dev) if blocks & MMD_XY else None
    ws = _run("am_mmd_rbf_cells_f32", dev, "am_mmd_rbf_cells_workspace_bytes", (pos[0], pos[1], d, blocks), _ptr(x), n, _ld(x),
              _opt(idx_x), pos[0], _host(host_ux), u1, _ptr(y), m, _ld(y), _opt(idx_y), pos[1], _host(host_uy), u2, d, bw2_arg,
              gamma_arg, blocks, _opt(xx), _opt(yy), _opt(xy))
    if idx_x is not None or idx_y is not None:
        flag = int(ws[:8].view(torch.int64).item())
        if flag != 0:
            p = flag - 1
            found = [f"{name}[{p}] = {int(idx[p].item())} (outside [0, {rows}))" for idx, rows, name in
                     ((idx_x, n, "idx_x"), (idx_y, m, "idx_y"))
                     if idx is not None and p < idx.numel() and not -1 <= int(idx[p].item()) < rows]
            raise ValueError("mmd_rbf_cell_sums: " + " / ".join(found) + ": positions are named by stored-row index, -1 marks an "
                             "empty one")
    return xx, yy, xy


MMD_KERNELS = {"gaussian": 0, "laplacian": 1, "energy": 2}        # enum am_mmd_kernel
MMD_MULTI_MAX = 4                                                    # AM_MMD_MULTI_MAX: scales per library call


def mmd_scales(scales):
    """The scale grid as a list of finite positive floats (at least one), or ValueError."""
    try:
        grid = [float(c) for c in scales]
    except TypeError:
        raise ValueError(f"scales must be a sequence of numbers, got {scales!r}") from None
    if not grid:
        raise ValueError("scales is empty: at least one scale is needed")
    for c in grid:
        if not (c > 0.0 and c < float("inf")):
            raise ValueError(f"scales must be finite and positive, got {c!r}")
    return grid


def _side_bandwidth(kernel, bw2, name):
    """(device pointer, host value) of a squared bandwidth `name` of the `kernel` family: a float32 device scalar or a number;
    the "energy" kernel has none."""
    if kernel == "energy":
        return ctypes.c_void_p(None), 0.0
    if bw2 is None:
        raise ValueError(f'the "{kernel}" kernel needs {name} (a float32 device scalar or a number)')
    if torch.is_tensor(bw2):
        _require_cuda(bw2, name)
        if bw2.dtype != torch.float32 or bw2.numel() != 1:
            raise ValueError(f"{name} must be a float32 device scalar")
        return _ptr(bw2), 0.0
    host = float(bw2)
    if not (host > 0.0 and host < float("inf")):
        raise ValueError(f"{name}={bw2!r} must be finite and positive")
    return ctypes.c_void_p(None), host


def mmd_multi_sums(x, y, kernel, scales, bw2=None, blocks=7, out=None):
    """float64 [3, S] device tensor: row 0 Sxx, 1 Syy, 2 Sxy (ordered pairs i != j / all pairs, as mmd_rbf_sums) of S kernels
    of one family in one Gram pass per at most four scales (am_mmd_multi_f32).  `kernel`: "gaussian" exp(-d2 g),
    g = 0.5 / (bw2 c c); "laplacian" exp(-d h), h = 1 / (c sqrt(bw2)); "energy" -d (one scale, no bandwidth) - c running over
    `scales`.  `bw2`: a 0-dim float32 DEVICE tensor (the output of pairwise_select_sq, no host round trip) or a number.  The
    Gaussian column of scale c holds the bits of mmd_rbf_sums(gamma=0.5 / (bw2 * (c * c))); no column depends on the other
    scales or on where a longer grid is cut into calls.  Only the rows named by `blocks` are written; the others keep what
    `out` held (NaN in a fresh tensor).  float32 rows only; stream-ordered, nothing waits for the device."""
    if kernel not in MMD_KERNELS:
        raise ValueError(f"kernel={kernel!r} is not one of {sorted(MMD_KERNELS)}")
    grid = mmd_scales(scales)
    if kernel == "energy" and len(grid) != 1:
        raise ValueError(f'the "energy" kernel has no bandwidth: it takes one scale, got {len(grid)}')
    _check_gram_rows("mmd_multi_sums", x, y)
    blocks = _blocks_mask(blocks)
    bw2_arg, bw2_host = _side_bandwidth(kernel, bw2, "bw2")
    nscales = len(grid)
    x, y = as_matrix(x, "x"), as_matrix(y, "y")
    dev = _same_device(x, y)
    if out is None:
        out = torch.full((3, nscales), float("nan"), dtype=torch.float64, device=dev)
    elif not (out.device == dev and out.dtype == torch.float64 and tuple(out.shape) == (3, nscales) and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float64 [3, {nscales}] tensor on the device of the rows")
    (n, d), m = x.shape, y.shape[0]
    rows = [b for b in range(3) if blocks & (1 << b)]
    for first in range(0, nscales, MMD_MULTI_MAX):
        part = grid[first:first + MMD_MULTI_MAX]
        k = len(part)
        # the library writes a dense [3][k]: the whole of `out`, or a staging tensor whose named rows go to columns first .. first + k
        dst = out if k == nscales else torch.empty((3, k), dtype=torch.float64, device=dev)
        _run("am_mmd_multi_f32", dev, "am_mmd_multi_workspace_bytes", (n, m, d, k, blocks), _ptr(x), n, _ld(x), _ptr(y), m, _ld(y), d,
             MMD_KERNELS[kernel], bw2_arg, bw2_host, _host((ctypes.c_double * k)(*part)), k, blocks, _ptr(dst))
        if dst is not out:
            for b in rows:
                out[b, first:first + k].copy_(dst[b])
    return out


PAIR_DEPENDENCE_MIN_ROWS = 4                                         # the unbiased statistics divide by n - 3


def pair_dependence(x, y, kernel, bw2x=None, bw2y=None, perm=None):
    """Row sums of the product of two Gram matrices of PAIRED sets in one library call (am_pair_dependence_f32): row i of x
    [n, dx] belongs to row i of y [n, dy] - with `perm` (int64 device tensor [n]) to row perm[i] of y, addressed through the
    list, no gathered copy.  Returns (rows, sums), float64 device tensors: rows [n, 5] = {A_i, B_i, H_i, AA_i, BB_i} with
    A_i = sum_{j != i} a_ij, B_i = sum b_ij, H_i = sum a_ij b_ij, AA_i = sum a_ij^2, BB_i = sum b_ij^2, and sums [8] = their
    five totals, sum A_i B_i, the number of finite rows and the number of non-finite rows (whose values are NaN).  `kernel`:
    "energy" a = +|x_i - x_j| (distance covariance), "gaussian" exp(-d2 / (2 bw2)), "laplacian" exp(-d / sqrt(bw2)), with
    `bw2x` / `bw2y` the squared bandwidth of each side: a 0-dim float32 DEVICE tensor (the output of pairwise_select_sq, no
    host round trip) or a number.  float32 rows only; stream-ordered, nothing waits for the device."""
    if kernel not in MMD_KERNELS:
        raise ValueError(f"kernel={kernel!r} is not one of {sorted(MMD_KERNELS)}")
    _check_gram_rows("pair_dependence", x, y, widths=False)
    if x.shape[0] != y.shape[0]:
        raise ValueError(f"row counts differ: {x.shape[0]} and {y.shape[0]} (row i of x belongs to row i of y)")
    n = int(x.shape[0])
    if n < PAIR_DEPENDENCE_MIN_ROWS:
        raise ValueError(f"{n} paired rows: the unbiased statistics need at least {PAIR_DEPENDENCE_MIN_ROWS}")
    if x.shape[1] < 1 or y.shape[1] < 1:
        raise ValueError(f"feature widths {x.shape[1]} and {y.shape[1]} must be at least 1")
    if perm is not None and (not torch.is_tensor(perm) or perm.dim() != 1 or perm.numel() != n or perm.dtype != torch.int64):
        raise ValueError(f"perm must be an int64 tensor of the {n} row indices of y")
    if x.device != y.device or (perm is not None and perm.device != x.device):
        raise ValueError("x, y and perm must be on one device")
    (bwx_arg, bwx_host), (bwy_arg, bwy_host) = _side_bandwidth(kernel, bw2x, "bw2x"), _side_bandwidth(kernel, bw2y, "bw2y")
    x, y = as_matrix(x, "x"), as_matrix(y, "y")
    dev = _same_device(x, y)
    if perm is not None:
        _require_cuda(perm, "perm")
        perm = perm.contiguous()
    rows = torch.empty((n, 5), dtype=torch.float64, device=dev)
    sums = torch.empty(8, dtype=torch.float64, device=dev)
    _run("am_pair_dependence_f32", dev, "am_pair_dependence_workspace_bytes", (n, x.shape[1], y.shape[1]), _ptr(x), n, _ld(x),
         x.shape[1], _ptr(y), _ld(y), y.shape[1], _opt(perm), MMD_KERNELS[kernel], bwx_arg, bwx_host, bwy_arg, bwy_host, _ptr(rows),
         _ptr(sums))
    return rows, sums


def mmd_rbf_group_sums(x, idx, offsets, y, bw2=None, gamma=None, rows=False):
    """Per-group Gaussian kernel sums in one library call (am_mmd_rbf_groups_f32; both sets float64:
    am_mmd_rbf_groups_f64): group b is the rows
    x[idx[offsets[b]:offsets[b + 1]]] (idx: int64 device tensor, or None for the rows in stored order; offsets: B + 1 host
    integers starting at 0, strictly increasing; any group size), each against the whole reference y.  `bw2` / `gamma` as
    for mmd_rbf_sums.  Nothing waits for the device: returns (out_groups, check), or (out_groups, out_rows, check) with
    rows=True - out_groups the f64 device tensor [B, 2] of {Sxx_b, Sxy_b} (Sxx_b over the ordered pairs i != j inside the
    group, Sxy_b over all n_b N2 pairs), out_rows the f64 device tensor [n_total, 2] of the row sums {w_i, c_i} in LIST
    order, and check() the one host read of the workspace's flag word, which raises ValueError for an index outside
    [0, N1) (the kernels never dereference it)."""
    f64 = _both_f64("mmd_rbf_group_sums", x, y)
    bw2_arg, gamma_arg = _bandwidth_args(bw2, gamma)
    (x, ldx, kind), (y, ldy, _) = _rows(x, "x", f64), _rows(y, "y", f64)
    dev = _same_device(x, y)
    n, d = x.shape
    if d != y.shape[1]:
        raise ValueError(f"feature widths differ: {d} and {y.shape[1]}")
    offs, b, host_offs = _group_offsets(offsets)
    idx = _group_index(idx, offs[-1], x)
    out_groups = torch.empty((b, 2), dtype=torch.float64, device=dev)
    out_rows = torch.empty((offs[-1], 2), dtype=torch.float64, device=dev) if rows else None
    ws = _run("am_mmd_rbf_groups_" + kind, dev, _query("mmd_rbf_groups", f64), (offs[-1], b, y.shape[0], d), _ptr(x), n, ldx,
              _opt(idx), _host(host_offs), b, _ptr(y), y.shape[0], ldy, d, bw2_arg, gamma_arg, _ptr(out_groups), _opt(out_rows))
    check = _index_check(ws, idx, n, "group rows")
    return (out_groups, out_rows, check) if rows else (out_groups, check)


# ------------------------------------------------------------------ PRDC
class PreparedSet:
    """What every PRDC entry point derives from a set before its tile kernels run - squared row norms, their maximum, the
    largest |element| and the scaled f16 copy (am_prepare_set_f32) - computed once and handed to the *_prepared_* entry
    points.  `rows(lo, hi)` is the prepared form of a row shard (same statistics, offset pointers)."""

    def __init__(self, norms, stats, half, ld_half, source):
        self.norms, self.stats, self.half, self.ld_half = norms, stats, half, ld_half
        self.source = source                      # (data_ptr, n, d) of the matrix it was prepared from

    def matches(self, x):
        return self.source == (x.data_ptr(), x.shape[0], x.shape[1])

    def rows(self, lo, hi):
        return PreparedSet(self.norms[lo:hi], self.stats, self.half[lo * self.ld_half:hi * self.ld_half], self.ld_half,
                           (self.source[0] + 0, hi - lo, self.source[2]))

    def struct(self):
        return _lib.PreparedSetStruct(self.norms.data_ptr(), self.stats.data_ptr(), self.half.data_ptr())


def prepare(x):
    """PreparedSet of a float32 set; None for float64 rows (the f64 kernels derive nothing ahead of their tile loop)."""
    if is_f64(x):
        return None
    lib = _lib.load()
    x = as_matrix(x)
    n, d = x.shape
    ldh = int(lib.am_prepared_half_ld(d))
    norms = torch.empty(n, dtype=torch.float32, device=x.device)
    stats = torch.empty(4, dtype=torch.int32, device=x.device)
    half = torch.empty(n * ldh, dtype=torch.int16, device=x.device)
    _call(lib, "am_prepare_set_f32", x.device, _ptr(x), n, _ld(x), d, _ptr(norms), _ptr(stats), _ptr(half))
    return PreparedSet(norms, stats, half, ldh, (x.data_ptr(), n, d))


def knn_radii(x, k, columns=None, prepared=None):
    """(k+1)-th smallest distance from each row of x to the rows of `columns`
    (default: x itself) - prdc.py:4-14, in the dtype of the rows (float64 rows: float64 radii, am_knn_radii_f64).
    `prepared`: the PreparedSet of x (self-distance form of float32 sets only)."""
    f64 = _any_f64(x, columns)
    x, ldx, kind = _rows(x, "embeddings", f64)
    y, ldy = (x, ldx) if columns is None else _rows(columns, "columns", f64)[:2]
    n, d = x.shape
    if y.shape[1] != d:
        raise ValueError("feature dimensions differ")
    out = torch.empty(n, dtype=x.dtype, device=x.device)
    query = _query("knn", f64), (n, y.shape[0], d, int(k))
    if prepared is not None and columns is None and not f64:
        ps = prepared.struct()
        _run("am_knn_radii_prepared_f32", x.device, *query, _ptr(x), n, ldx, d, ctypes.byref(ps), int(k), _ptr(out))
    else:
        _run("am_knn_radii_" + kind, x.device, *query, _ptr(x), n, ldx, _ptr(y), y.shape[0], ldy, d, int(k), _ptr(out))
    return out


KNN_SEARCH_MAX_K = 32


def _check_row_labels(x, y, x_group, y_group):
    """The labels of the leave-group-out ops: int32 tensors, one label per row, on the device of their rows."""
    for labels, rows, name in ((x_group, x, "x_group"), (y_group, y, "y_group")):
        if not torch.is_tensor(labels) or labels.dtype != torch.int32:
            raise ValueError(f"{name} must be an int32 tensor, got {getattr(labels, 'dtype', type(labels).__name__)}")
        if labels.dim() != 1 or labels.shape[0] != rows.shape[0]:
            raise ValueError(f"{name} must hold one label per row: shape {tuple(labels.shape)} for {rows.shape[0]} rows")
        if labels.device != rows.device:
            raise ValueError(f"{name} lives on {labels.device}, its rows on {rows.device}")


def _knn_search(op, x, y, k, squared, self_offset=None, groups=None):
    """knn_search (groups is None: exclusion by index) and knn_search_groups (groups = (x_group, y_group)); `op` names the
    caller in the messages."""
    _refuse_f64(op, x, y)
    k = int(k)
    if not 1 <= k <= KNN_SEARCH_MAX_K:
        raise ValueError(f"k={k} must be in 1 .. {KNN_SEARCH_MAX_K}")
    _check_two_sets(op, x, y, sides=False)
    if x.shape[0] < 1 or y.shape[0] < 1:
        raise ValueError(f"{op} needs rows on both sides (got {x.shape[0]} and {y.shape[0]})")
    if groups is not None:
        _check_row_labels(x, y, *groups)
    x, y, dev, n, m, d = _two_sets(x, y)
    dist = torch.empty((n, k), dtype=torch.float32, device=dev)
    idx = torch.empty((n, k), dtype=torch.int64, device=dev)
    out = (1 if squared else 0, _ptr(dist), _ptr(idx))
    if groups is None:
        _run("am_knn_search_f32", dev, "am_knn_search_workspace_bytes", (n, m, d, k), _ptr(x), n, _ld(x), _ptr(y), m, _ld(y), d, k,
             -1 if self_offset is None else int(self_offset), *out)
    else:
        x_group, y_group = (g.contiguous() for g in groups)
        _run("am_knn_search_groups_f32", dev, "am_knn_search_groups_workspace_bytes", (n, m, d, k), _ptr(x), n, _ld(x), _ptr(x_group),
             _ptr(y), m, _ld(y), _ptr(y_group), d, k, *out)
    return dist, idx


def knn_search(x, y, k, self_offset=None, squared=False):
    """The k nearest rows of y for every row of x (am_knn_search_f32): (dist float32 [N, k] ascending, idx int64 [N, k]) as
    device tensors, stream-ordered, nothing waits for the device.  Squared distances have the bits of the exact k-NN kernel
    (column k of a (k + 1)-search is knn_radii(x, k, columns=y)); ties go to the smallest row index of y; `self_offset`:
    column i + self_offset is skipped for row i (0 for x searched against itself, the shard's first row for a row shard),
    by index - duplicate rows stay neighbours.  Missing neighbours (fewer than k finite candidates) are (+inf, -1)."""
    return _knn_search("knn_search", x, y, k, squared, self_offset=self_offset)


def knn_search_groups(x, y, k, x_group, y_group, squared=False):
    """The k nearest rows of y WITH ANOTHER LABEL for every row of x (am_knn_search_groups_f32): row j of y is skipped for
    row i of x iff x_group[i] == y_group[j] - int32 device vectors, one label per row, any values.  Everything else is
    knn_search: (dist float32 [N, k] ascending, idx int64 [N, k]) as device tensors, stream-ordered, nothing waits for the
    device; the bits of knn_search's distances; ties go to the smallest row index of y; (+inf, -1) where a row has fewer
    than k admissible finite candidates.  A set searched against itself with its own labels leaves out each row's whole
    group, the row included."""
    return _knn_search("knn_search_groups", x, y, k, squared, groups=(x_group, y_group))


def knn_search_chunks(n, m, d, k):
    """Column chunks the search's plan cuts the rows of y into (am_knn_search_chunks; tests and tools)."""
    return int(_lib.load().am_knn_search_chunks(int(n), int(m), int(d), int(k)))


# ---- per-sample realism, ball count and rarity on the PRDC manifold (csrc/sample_scores.hip) ----
def _sample_scores(op, x, y, r_y, groups=None):
    """sample_scores (groups is None: every pair counts) and sample_scores_groups (groups = (x_group, y_group)); `op` names
    the caller in the messages."""
    _refuse_f64(op, x, y, r_y)
    _check_two_sets(op, x, y)
    if not torch.is_tensor(r_y) or r_y.dim() != 1 or r_y.shape[0] != y.shape[0] or r_y.dtype != torch.float32:
        raise ValueError(f"r_y must be a float32 tensor with one radius per row of y ({y.shape[0]}), got "
                         f"{tuple(r_y.shape) if torch.is_tensor(r_y) else type(r_y).__name__}"
                         f"{' ' + str(r_y.dtype) if torch.is_tensor(r_y) else ''}")
    if groups is not None:
        _check_row_labels(x, y, *groups)
    x, y, dev, n, m, d = _two_sets(x, y, more=((r_y, "r_y"),))
    r_y = r_y.contiguous()
    realism = torch.empty(n, dtype=torch.float32, device=dev)
    realism_idx = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    rarity = torch.empty(n, dtype=torch.float32, device=dev)
    rarity_idx = torch.empty(n, dtype=torch.int64, device=dev)
    out = (_ptr(r_y), _ptr(realism), _ptr(realism_idx), _ptr(count), _ptr(rarity), _ptr(rarity_idx))
    if groups is None:
        _run("am_sample_scores_f32", dev, "am_sample_scores_workspace_bytes", (n, m, d), _ptr(x), n, _ld(x), _ptr(y), m, _ld(y), d, *out)
    else:
        x_group, y_group = (g.contiguous() for g in groups)
        _run("am_sample_scores_groups_f32", dev, "am_sample_scores_groups_workspace_bytes", (n, m, d), _ptr(x), n, _ld(x), _ptr(x_group),
             _ptr(y), m, _ld(y), _ptr(y_group), d, *out)
    return realism, realism_idx, count, rarity, rarity_idx


def sample_scores(x, y, r_y):
    """Realism, ball count and rarity of every row of x against the rows of y and their k-NN radii r_y
    (am_sample_scores_f32): (realism float32 [N], realism_index int64 [N], ball_count int32 [N], rarity float32 [N],
    rarity_index int64 [N]) as device tensors, stream-ordered, nothing waits for the device.  realism = max_j r_j / |x - y_j|
    (+inf on a row of y with a positive radius), ball_count = the balls the row lies in, with the bits of
    prdc_counts(y, x, r_y, .)[0], rarity = the smallest radius among those balls (0 outside every ball); indices name rows
    of y, ties go to the smallest, -1 where there is none.  A radius that is not > 0 is nobody's ball."""
    return _sample_scores("sample_scores", x, y, r_y)


def sample_scores_chunks(n, m, d):
    """Column chunks the plan cuts the rows of y into (am_sample_scores_chunks; tests and tools)."""
    return int(_lib.load().am_sample_scores_chunks(int(n), int(m), int(d)))


def sample_scores_groups(x, y, r_y, x_group, y_group):
    """sample_scores over the pairs of DIFFERENT labels (am_sample_scores_groups_f32): row j of y is no reference row of
    row i of x iff x_group[i] == y_group[j] - int32 device vectors, one label per row, any values - so it is not counted,
    its ratio is 0 and it is no candidate of the rarity.  Everything else is sample_scores: the same five device tensors
    (realism float32 [N], realism_index int64 [N], ball_count int32 [N], rarity float32 [N], rarity_index int64 [N]),
    stream-ordered, nothing waits for the device; the bits of sample_scores on the admissible columns; ties go to the
    smallest row index of y; (0, -1, 0, 0.0, -1) for a row with no admissible reference row.  A set scored against itself
    with its own labels scores every row against the other groups."""
    return _sample_scores("sample_scores_groups", x, y, r_y, groups=(x_group, y_group))


# ---- probabilistic scoring rule of a point against a set (csrc/psr.hip) ----
PSR_RADIUS_SQ_MAX = 3.4028234663852886e+38                     # FLT_MAX: the in-range threshold is a float32


def psr_scores(x, y, radius, sums=True):
    """PSR and in-range count of every row of x against the rows of y and ONE radius of the set y (am_psr_f32):
    (psr float64 [N], count int32 [N], sums float64 [2] or None) as device tensors, stream-ordered, nothing waits for the
    device.  count = #{ j : |x - y_j| < radius }, psr = 1 - prod over those j of |x - y_j| / radius (0.0 with nothing in
    range, 1.0 on a row of y); sums = { sum psr, sum count } in a fixed tree (sums=False: not computed).  The squared
    distances have the bits of knn_search(x, y, ., squared=True); `x is y` computes the norms once.  Two calls at the same
    shapes return the same bits; the last bits of psr depend on the chunk plan (psr_chunks)."""
    _refuse_f64("psr_scores", x, y)
    _check_two_sets("psr_scores", x, y)
    radius = float(radius)
    if not (math.isfinite(radius) and radius > 0.0 and radius * radius <= PSR_RADIUS_SQ_MAX):
        raise ValueError(f"radius={radius} must be finite and > 0, with radius^2 a finite float32 number")
    x, y, dev, n, m, d = _two_sets(x, y)
    psr = torch.empty(n, dtype=torch.float64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.float64, device=dev) if sums else None
    _run("am_psr_f32", dev, "am_psr_workspace_bytes", (n, m, d), _ptr(x), n, _ld(x), _ptr(y), m, _ld(y), d, radius, _ptr(psr),
         _ptr(count), _opt(totals))
    return psr, count, totals


def psr_chunks(n, m, d):
    """Column chunks the plan cuts the rows of y into (am_psr_chunks; tests and tools)."""
    return int(_lib.load().am_psr_chunks(int(n), int(m), int(d)))


# ---- retrieval ranks of paired sets (csrc/retrieval.hip) ----
def _check_segments(q, pos_start, pos_count, pos_columns):
    """The positives of retrieval_ranks: int64 tensors on the device of the rows, one start and one count per query row."""
    for t, name in ((pos_start, "pos_start"), (pos_count, "pos_count"), (pos_columns, "pos_columns")):
        if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1:
            raise ValueError(f"{name} must be a 1-D int64 tensor, got {getattr(t, 'dtype', type(t).__name__)}"
                             f"{' of shape ' + str(tuple(t.shape)) if torch.is_tensor(t) else ''}")
        if t.device != q.device:
            raise ValueError(f"{name} lives on {t.device}, the rows on {q.device}")
    for t, name in ((pos_start, "pos_start"), (pos_count, "pos_count")):
        if t.shape[0] != q.shape[0]:
            raise ValueError(f"{name} must hold one entry per query row: {t.shape[0]} for {q.shape[0]} rows")


def retrieval_ranks(q, g, pos_start, pos_count, pos_columns, cosine=True, groups=None):
    """The rank of every query row's best positive among the rows of g (am_retrieval_ranks_f32): (better int32 [N], tied
    int32 [N], score float32 [N], positive int64 [N], n_pos int32 [N], n_pos_own_group int32 [N]) as device tensors,
    stream-ordered, nothing waits for the device.  The positives of row i are the columns
    pos_columns[pos_start[i] : pos_start[i] + pos_count[i]] (int64 device tensors; distinct columns inside a segment).  A
    pair scores u = <q_i, g_j> * w_j with the bits of the exact tile engine, w_j = 1 / |g_j| (cosine) or 1 (dot), correctly
    rounded; a NaN u is no score.  t = the best scored positive, `positive` the smallest column reaching it, better / tied =
    the negatives with u > t / u == t, score = t (dot) or the cosine itself; rank = 1 + better.  A row without a scored
    positive, or with a positive outside [0, M), is unranked: (-1, -1, NaN, -1).  groups = (q_group, g_group), int32 device
    vectors: a column of the row's own group is no negative (a positive there is still a positive).  `q is g` computes the
    norms once.  Two calls return the same bits."""
    _refuse_f64("retrieval_ranks", q, g)
    _check_two_sets("retrieval_ranks", q, g, both="q and g")
    if groups is not None:
        _check_row_labels(q, g, *groups)
    q, g, dev, n, m, d = _two_sets(q, g, ("q", "g"))
    _check_segments(q, pos_start, pos_count, pos_columns)
    pos_start, pos_count, pos_columns = pos_start.contiguous(), pos_count.contiguous(), pos_columns.contiguous()
    better = torch.empty(n, dtype=torch.int32, device=dev)
    tied = torch.empty(n, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    positive = torch.empty(n, dtype=torch.int64, device=dev)
    n_pos = torch.empty(n, dtype=torch.int32, device=dev)
    n_pos_own = torch.empty(n, dtype=torch.int32, device=dev)
    q_group, g_group = (t.contiguous() for t in groups) if groups is not None else (None, None)
    _run("am_retrieval_ranks_f32", dev, "am_retrieval_workspace_bytes", (n, m, d), _ptr(q), n, _ld(q), _ptr(g), m, _ld(g), d,
         1 if cosine else 0, _ptr(pos_start), _ptr(pos_count), _opt(pos_columns if pos_columns.numel() else None),
         int(pos_columns.numel()), _opt(q_group), _opt(g_group), _ptr(better), _ptr(tied), _ptr(score), _ptr(positive), _ptr(n_pos),
         _ptr(n_pos_own))
    return better, tied, score, positive, n_pos, n_pos_own


def retrieval_chunks(n, m, d):
    """Column chunks the plan cuts the rows of g into (am_retrieval_chunks; tests and tools)."""
    return int(_lib.load().am_retrieval_chunks(int(n), int(m), int(d)))


# ---- k-means: the two halves of a Lloyd iteration (csrc/kmeans.hip) ----
def _kmeans_check(what, x, c):
    _refuse_f64(what, x, c)
    _check_two_sets(what, x, c, both="rows and centroids", sides=False)
    if c.shape[0] < 1:
        raise ValueError(f"{what} needs at least one centroid (K={c.shape[0]})")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what} needs rows (got shape {tuple(x.shape)})")


def kmeans_assign(x, c):
    """The nearest row of c for every row of x (am_kmeans_assign_f32): (labels int64 [N], d2 float32 [N], inertia float64
    0-d) as device tensors, stream-ordered, nothing waits for the device.  labels and d2 have the bits of
    knn_search(x, c, 1, squared=True); ties go to the smallest centroid index; a row without a finite distance is
    (-1, +inf) and is left out of inertia, the f64 sum of d2 added in a fixed order."""
    _kmeans_check("kmeans_assign", x, c)
    x, c, dev, n, k, d = _two_sets(x, c, ("x", "c"))
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    d2 = torch.empty(n, dtype=torch.float32, device=dev)
    inertia = torch.empty((), dtype=torch.float64, device=dev)
    _run("am_kmeans_assign_f32", dev, "am_kmeans_assign_workspace_bytes", (n, k, d), _ptr(x), n, _ld(x), _ptr(c), k, _ld(c), d,
         _ptr(labels), _ptr(d2), _ptr(inertia))
    return labels, d2, inertia


def kmeans_update(x, labels, c_old):
    """The mean of the rows of x under every label (am_kmeans_update_f32): (c_new float32 [K, D], counts int64 [K]) as
    device tensors, stream-ordered, nothing waits for the device.  Sums run in f64 in ascending row order and are rounded to
    f32 once; a label without rows keeps its row of c_old bit for bit and counts 0; labels of -1 (kmeans_assign's "no finite
    distance") are ignored.  The rows are sorted by label on the device (torch.sort(stable=True), torch.searchsorted)."""
    _kmeans_check("kmeans_update", x, c_old)
    if not torch.is_tensor(labels) or labels.dim() != 1 or labels.shape[0] != x.shape[0] or labels.dtype != torch.int64:
        raise ValueError(f"labels must be an int64 tensor with one entry per row ({x.shape[0]}), got "
                         f"{getattr(labels, 'dtype', type(labels).__name__)} {tuple(getattr(labels, 'shape', ()))}")
    x, c_old, dev, n, k, d = _two_sets(x, c_old, ("x", "c_old"), more=((labels, "labels"),))
    labels = labels.contiguous()
    ordered, order = torch.sort(labels, stable=True)                       # rows with label -1 come first
    offsets = torch.searchsorted(ordered, torch.arange(k + 1, dtype=torch.int64, device=dev))
    ld = (d + 3) // 4 * 4
    c_new = torch.empty((k, ld), dtype=torch.float32, device=dev)[:, :d]
    counts = torch.empty(k, dtype=torch.int64, device=dev)
    _run("am_kmeans_update_f32", dev, "am_kmeans_update_workspace_bytes", (n, k, d), _ptr(x), n, _ld(x), d, _ptr(labels), _ptr(order),
         _ptr(offsets), k, _ptr(c_old), _ld(c_old), _ptr(c_new), ld, _ptr(counts))
    return c_new, counts


# ---- soft-min: one log-domain Sinkhorn half-step (csrc/softmin.hip) ----
def _potential_ok(t, rows):
    return t is None or (torch.is_tensor(t) and t.dim() == 1 and t.shape[0] == rows and t.dtype == torch.float64)


def softmin(x, y, g=None, eps=None, prev=None, damping=0.0):
    """T_i = -eps log((1 / M) sum_j exp((g_j - |x_i - y_j|^2 / 2) / eps)) for every row of x against the M rows of y
    (am_softmin_f32): (out float64 [N], change float64 0-d, magnitude float64 0-d) as device tensors, stream-ordered, nothing
    waits for the device.  g: float64 [M] potentials on the rows of y (None: zeros); out = damping * prev + (1 - damping) * T
    (damping == 0: T itself); change = max |out - prev| (prev None: max |out|), magnitude = max |out|.  The squared
    distances have the bits of knn_search(x, y, ., squared=True); `x is y` computes the norms once.  Two calls return the
    same bits."""
    _refuse_f64("softmin", x, y)
    _check_two_sets("softmin", x, y)
    if eps is None or not math.isfinite(float(eps)) or float(eps) <= 0.0:
        raise ValueError(f"eps={eps!r} must be a finite positive number")
    eps, damping = float(eps), float(damping)
    if not 0.0 <= damping < 1.0:
        raise ValueError(f"damping={damping!r} must lie in [0, 1)")
    if not _potential_ok(g, y.shape[0]):
        raise ValueError(f"g must be a float64 tensor with one potential per row of y ({y.shape[0]})")
    if not _potential_ok(prev, x.shape[0]):
        raise ValueError(f"prev must be a float64 tensor with one value per row of x ({x.shape[0]})")
    if damping != 0.0 and prev is None:
        raise ValueError(f"damping={damping!r} needs prev")
    x, y, dev, n, m, d = _two_sets(x, y, more=[(t, name) for t, name in ((g, "g"), (prev, "prev")) if t is not None])
    g = g.contiguous() if g is not None else None
    prev = prev.contiguous() if prev is not None else None
    out = torch.empty(n, dtype=torch.float64, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    _run("am_softmin_f32", dev, "am_softmin_workspace_bytes", (n, m, d), _ptr(x), n, _ld(x), _ptr(y), m, _ld(y), d, _opt(g), eps,
         _opt(prev), damping, _ptr(out), _ptr(stats))
    return out, stats[0], stats[1]


# ---- feature likelihood of a mixture of isotropic Gaussians: the loglik sweep and the gradient sweep (csrc/fld.hip) ----
FLD_THETA_MAX = 30.0                                   # upper clamp of theta = log sigma^2 (csrc/fld.hip: THETA_MAX)
FLD_THETA_MIN_LIMIT = -math.log(2.0 * 3.4028234663852886e38)      # below it 0.5 exp(-theta) is no finite float32 number


def _fld_vector_ok(t, rows):
    return torch.is_tensor(t) and t.dim() == 1 and t.shape[0] == rows and t.dtype == torch.float64


def fld_loglik(x, g, theta, stats=None):
    """l_i = logsumexp_j (-h_j d2(x_i, g_j) - c_j) - log M - (D / 2) log 2 pi for every row of x under the mixture of
    isotropic Gaussians on the M rows of g with log-variances theta (float64 [M]; h = 0.5 exp(-theta), c = (D / 2) theta)
    (am_fld_loglik_f32): (loglik float64 [N], stats float64 [3] = {sum of the finite l, rows with a finite l, rows without})
    as device tensors, stream-ordered, nothing waits for the device.  `stats`: a contiguous float64 [3] device tensor to
    write the three numbers into (a row of a fit's history).  The squared distances have the bits of
    knn_search(x, g, ., squared=True); a row with a non-finite element has l = -inf, a centre with one contributes 0.  Two
    calls return the same bits."""
    _refuse_f64("fld_loglik", x, g)
    _check_two_sets("fld_loglik", x, g, both="x and g")
    if not _fld_vector_ok(theta, g.shape[0]):
        raise ValueError(f"theta must be a float64 tensor with one log-variance per row of g ({g.shape[0]})")
    if stats is not None and not (_fld_vector_ok(stats, 3) and stats.is_contiguous()):
        raise ValueError("stats must be a contiguous float64 tensor of 3 elements")
    x, g, dev, n, m, d = _two_sets(x, g, ("x", "g"), more=[(theta, "theta")] + ([] if stats is None else [(stats, "stats")]))
    theta = theta.contiguous()
    out = torch.empty(n, dtype=torch.float64, device=dev)
    if stats is None:
        stats = torch.empty(3, dtype=torch.float64, device=dev)
    _run("am_fld_loglik_f32", dev, "am_fld_loglik_workspace_bytes", (n, m, d), _ptr(x), n, _ld(x), _ptr(g), m, _ld(g), d, _ptr(theta),
         _ptr(out), _ptr(stats))
    return out, stats


def fld_grad_step(g, x, theta, lse, n_finite, m, v, step, lr, theta_min):
    """One full-batch Adam step on the log-variances theta of the mixture on the rows of g, fitted to the rows of x
    (am_fld_grad_f32): (theta, m, v, A, B), new float64 [M] device tensors, stream-ordered, nothing waits for the device - the
    arguments are left as they are.  lse: float64 [N], the loglik of fld_loglik(x, g, theta); n_finite: a float64 device
    tensor of one element, its stats[1].  A_j = sum_i r_ij and B_j = sum_i r_ij d2_ij over the responsibilities r_ij; the
    gradient is -(h_j B_j - (D / 2) A_j) / n_finite and the update that of metrics.fld.fld_adam_step with step >= 1, clamped
    to [theta_min, 30].  Two calls return the same bits."""
    _refuse_f64("fld_grad_step", x, g)
    _check_two_sets("fld_grad_step", x, g, both="x and g")
    for t, name, rows in ((theta, "theta", g.shape[0]), (m, "m", g.shape[0]), (v, "v", g.shape[0]), (lse, "lse", x.shape[0])):
        if not _fld_vector_ok(t, rows):
            raise ValueError(f"{name} must be a float64 tensor of {rows} elements")
    if not (torch.is_tensor(n_finite) and n_finite.dtype == torch.float64 and n_finite.numel() == 1):
        raise ValueError("n_finite must be a float64 tensor of one element (stats[1] of fld_loglik)")
    step, lr, theta_min = int(step), float(lr), float(theta_min)
    if step < 1:
        raise ValueError(f"step={step} must be at least 1")
    if not math.isfinite(lr) or lr < 0.0:
        raise ValueError(f"lr={lr!r} must be finite and not negative")
    if not math.isfinite(theta_min) or not FLD_THETA_MIN_LIMIT <= theta_min <= FLD_THETA_MAX:
        raise ValueError(f"theta_min={theta_min!r} must lie in [{FLD_THETA_MIN_LIMIT:.4f}, {FLD_THETA_MAX}]: "
                         "0.5 exp(-theta) has to stay a normal float32 number")
    vectors = ((theta, "theta"), (lse, "lse"), (n_finite, "n_finite"), (m, "m"), (v, "v"))
    g, x, dev, rows, n, d = _two_sets(g, x, ("g", "x"), more=vectors)
    theta, lse, n_finite, m, v = (t.contiguous() for t, _ in vectors)
    m, v = m.clone(), v.clone()                                      # the kernel updates its moments in place
    theta_out, a, b = (torch.empty(rows, dtype=torch.float64, device=dev) for _ in range(3))
    _run("am_fld_grad_f32", dev, "am_fld_grad_workspace_bytes", (rows, n, d), _ptr(g), rows, _ld(g), _ptr(x), n, _ld(x), d, _ptr(theta),
         _ptr(lse), _ptr(n_finite), _ptr(m), _ptr(v), step, lr, theta_min, _ptr(theta_out), _ptr(a), _ptr(b))
    return theta_out, m, v, a, b


# ---- sliced Wasserstein distance: project, sort, transport cost (csrc/swd.hip) ----
def sliced_project(x, theta):
    """z[l, i] = <theta_l, x_i> for the rows of x [N, D] and the directions theta [L, D] (am_sliced_project_f32): float32
    [L, N] as a device tensor, stream-ordered, nothing waits for the device.  A projection's bits do not depend on which
    other directions share the call."""
    _refuse_f64("sliced_project", x, theta)
    _check_two_sets("sliced_project", x, theta, both="rows and directions", sides=False)
    if x.shape[0] < 1 or theta.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"sliced_project needs rows and directions (got shapes {tuple(x.shape)} and {tuple(theta.shape)})")
    lib = _lib.load()
    x, theta = as_matrix(x, "x"), as_matrix(theta, "theta")
    dev = _same_device(x, theta)
    n, d = x.shape
    nl = theta.shape[0]
    z = torch.empty((nl, n), dtype=torch.float32, device=dev)
    _call(lib, "am_sliced_project_f32", dev, _ptr(x), n, _ld(x), _ptr(theta), nl, _ld(theta), d, _ptr(z), n)
    return z


def _sorted_matrix(z, name):
    _refuse_f64(name, z)
    if not torch.is_tensor(z) or z.dim() != 2 or z.shape[0] < 1 or z.shape[1] < 1:
        raise ValueError(f"{name} needs a 2-D tensor with rows and columns (got {tuple(getattr(z, 'shape', ()))})")


def _unit_columns(z, name):
    """float32, unit column stride, rows that do not overlap: what the key kernels address (any row stride >= columns)."""
    _require_cuda(z, name)
    if z.dtype != torch.float32 or z.stride(1) != 1 or (z.shape[0] > 1 and z.stride(0) < z.shape[1]):
        z = z.to(torch.float32).contiguous()
    return z


def _row_stride(z):
    return z.stride(0) if z.shape[0] > 1 else z.shape[1]


def sort_rows(z, out=None):
    """Every row of z [L, N] sorted ascending, keys only (am_sort_rows_f32): float32 [L, N] as a device tensor, stream-ordered,
    nothing waits for the device.  -0.0 before +0.0, NaNs last as the canonical quiet NaN.  out=z sorts in place (z must then
    be float32 with unit column stride); the workspace is one more [L, N] matrix."""
    _sorted_matrix(z, "sort_rows")
    src = _unit_columns(z, "z")
    if out is None:
        out = torch.empty(tuple(src.shape), dtype=torch.float32, device=src.device)
    elif out is z:
        if src is not z:
            raise ValueError("sort_rows: an in-place sort needs a float32 tensor with unit column stride")
    else:
        raise ValueError("sort_rows: out must be None or z itself")
    nl, n = src.shape
    _run("am_sort_rows_f32", src.device, "am_sort_rows_workspace_bytes", (nl, n), _ptr(src), nl, n, _row_stride(src), _ptr(out),
         _row_stride(out))
    return out


def sliced_w(zx_sorted, zy_sorted, p=2):
    """W_p^p between row l of zx_sorted [L, n] and row l of zy_sorted [L, m], both sorted ascending, as uniform empirical
    measures (am_sliced_w_f32): (w float64 [L], nonfinite int32 [L]) as device tensors, stream-ordered, nothing waits for the
    device.  p is 1 or 2.  (zx, zy) and (zy, zx) return the same bits, a matrix against itself exactly 0.0; a row that holds
    a NaN or an infinity on either side gives NaN and its count."""
    _sorted_matrix(zx_sorted, "sliced_w")
    _sorted_matrix(zy_sorted, "sliced_w")
    if p not in (1, 2):
        raise ValueError(f"p={p!r} must be 1 or 2")
    if zx_sorted.shape[0] != zy_sorted.shape[0]:
        raise ValueError(f"the two sides hold {zx_sorted.shape[0]} and {zy_sorted.shape[0]} projections")
    n, m = int(zx_sorted.shape[1]), int(zy_sorted.shape[1])
    if n * m >= 1 << 53:
        raise ValueError(f"n * m = {n} * {m} must stay below 2^53 (the coupling's weights are exact integers)")
    same = zx_sorted is zy_sorted
    zx = _unit_columns(zx_sorted, "zx_sorted")
    zy = zx if same else _unit_columns(zy_sorted, "zy_sorted")
    dev = _same_device(zx, zy)
    nl = zx.shape[0]
    w = torch.empty(nl, dtype=torch.float64, device=dev)
    bad = torch.empty(nl, dtype=torch.int32, device=dev)
    _run("am_sliced_w_f32", dev, "am_sliced_w_workspace_bytes", (nl, n, m), _ptr(zx), n, _row_stride(zx), _ptr(zy), m, _row_stride(zy),
         nl, int(p), _ptr(w), _ptr(bad))
    return w, bad


# ---- random Fourier features of the Gaussian kernel and their moment matrix (csrc/rff.hip) ----
def rff_max_features():
    return _host_cap("am_rff_max_features")


def rff_moment_chunks(n, n_features):
    """The number of row chunks am_rff_moment_f32 folds for n rows and n_features frequencies (a host query)."""
    return int(_lib.load().am_rff_moment_chunks(int(n), int(n_features)))


def _rff_width_args(bw2, inv_bw):
    """The (inv_bw, bw2 pointer) arguments of the am_rff_* entry points from exactly one of a float32 device scalar holding a
    squared bandwidth and the number 1 / bandwidth; no device call."""
    if (bw2 is None) == (inv_bw is None):
        raise ValueError("exactly one of bw2 (device scalar) and inv_bw (number) must be given")
    if bw2 is None:
        inv_bw = float(inv_bw)
        if not (inv_bw > 0.0 and inv_bw < float("inf")):
            raise ValueError(f"inv_bw={inv_bw!r} must be a finite positive number")
        return inv_bw, ctypes.c_void_p(None)
    _require_cuda(bw2, "bw2")
    if bw2.dtype != torch.float32 or bw2.numel() != 1:
        raise ValueError("bw2 must be a float32 device scalar")
    return 0.0, _ptr(bw2)


def _rff_check_inputs(what, x, w):
    _refuse_f64(what, x, w)
    _check_two_sets(what, x, w, both="rows and frequencies", sides=False)
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what} needs rows (got shape {tuple(x.shape)})")
    if not 1 <= w.shape[0] <= rff_max_features():
        raise ValueError(f"{what} takes 1 .. {rff_max_features()} frequencies, got {w.shape[0]}")


def _rff_count_check(ws):
    """check() of the am_rff_* calls: the one host read of the int64 at the head of the workspace - the number of rows with
    a NaN or an infinity (their features are zeros)."""
    def check():
        return int(ws[:8].view(torch.int64).item())
    return check


def rff_features(x, w, bw2=None, inv_bw=None, row0=0, nrows=None, out=None, return_check=False):
    """The random Fourier features of rows [row0, row0 + nrows) of x [N, D] under the frequencies w [R, D]
    (am_rff_features_f32): the float64 device tensor f [2R, nrows], feature-major, f[l, i] = cos(a) / sqrt(R) and f[R + l, i] =
    sin(a) / sqrt(R) with a = (double) <w_l, x_(row0 + i)> * inv_bw - `inv_bw` a number, or `bw2` a float32 DEVICE scalar
    holding bw^2 (inv_bw = 1 / sqrt(bw2) is formed on the device, no host round trip).  Stream-ordered, nothing waits for the
    device.  A feature's bits depend neither on the other frequencies of the call nor on (row0, nrows); a row with a NaN or
    an infinity gives zeros.  out: a contiguous float64 [2R, ldo >= nrows] device tensor to write into (columns from nrows on
    are left as they are; it is returned as it is).  return_check=True: (f, check), check() the one host read of the number
    of non-finite rows."""
    _rff_check_inputs("rff_features", x, w)
    inv_arg, dev_arg = _rff_width_args(bw2, inv_bw)
    n_all = int(x.shape[0])
    row0 = int(row0)
    nrows = n_all - row0 if nrows is None else int(nrows)
    if row0 < 0 or nrows < 1 or row0 + nrows > n_all:
        raise ValueError(f"rows [{row0}, {row0} + {nrows}) are not inside [0, {n_all})")
    r = int(w.shape[0])
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float64 or out.dim() != 2 or out.shape[0] != 2 * r
                            or out.shape[1] < nrows or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float64 [2R = {2 * r}, >= {nrows}] device tensor")
    x, w = as_matrix(x, "x"), as_matrix(w, "w")
    dev = _same_device(x, w) if out is None else _same_device(x, w, out)
    if bw2 is not None:
        _same_device(x, bw2)
    d = x.shape[1]
    f = torch.empty((2 * r, nrows), dtype=torch.float64, device=dev) if out is None else out
    ws = _run("am_rff_features_f32", dev, "am_rff_features_workspace_bytes", (nrows,), _ptr(x), n_all, _ld(x), d, _ptr(w), r, _ld(w),
              row0, nrows, inv_arg, dev_arg, _ptr(f), int(f.shape[1]))
    return (f, _rff_count_check(ws)) if return_check else f


def rff_moment(x, w, bw2=None, inv_bw=None):
    """S = (1 / n) sum_i phi_i phi_i^T over all rows of x, phi_i the random Fourier features rff_features describes, as an f64
    device tensor [2R, 2R] (am_rff_moment_f32): exactly symmetric, trace 1; its non-zero eigenvalues approximate those of the
    Gaussian kernel's K / n.  Returns (s, check); nothing waits for the device.  check() is the one host read of the number
    of rows with a NaN or an infinity (they count as zeros in s)."""
    _rff_check_inputs("rff_moment", x, w)
    inv_arg, dev_arg = _rff_width_args(bw2, inv_bw)
    x, w = as_matrix(x, "x"), as_matrix(w, "w")
    dev = _same_device(x, w)
    if bw2 is not None:
        _same_device(x, bw2)
    n, d = x.shape
    r = int(w.shape[0])
    s = torch.empty((2 * r, 2 * r), dtype=torch.float64, device=dev)
    ws = _run("am_rff_moment_f32", dev, "am_rff_moment_workspace_bytes", (n, d, r), _ptr(x), n, _ld(x), d, _ptr(w), r, _ld(w), inv_arg,
              dev_arg, _ptr(s))
    return s, _rff_count_check(ws)


# ---- classifier-output scores: row quantities of logits, per group or per row pair (csrc/class_scores.hip) ----
CLASS_GROUPS_MAX_COLUMNS = 2048                               # the column sums of a workgroup stay in LDS
ROW_PAIRS_MAX_COLUMNS = 8192
PAIR_MODES = {"cosine": 0, "kl_softmax": 1, "kl_sigmoid": 2, "kl_bernoulli": 3}      # enum am_pair_mode


def check_score_rows(t, name, cap):
    """The checks on a matrix of logits / embeddings that need no device: a 2-D float32 or float64 tensor with rows and
    1 .. cap columns."""
    if not torch.is_tensor(t) or t.dim() != 2:
        raise ValueError(f"{name} must be a 2-D tensor, got shape {tuple(getattr(t, 'shape', ()))}")
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be float32 or float64, got {t.dtype}")
    if t.shape[0] < 1 or not 1 <= t.shape[1] <= cap:
        raise ValueError(f"{name} has shape {tuple(t.shape)}: it needs rows and 1 .. {cap} columns")


def class_group_scores(rows, order, offsets, return_rows=False):
    """The Inception Score terms of every group of rows of logits (am_class_groups_f32 / _f64, by the dtype of rows; the
    group list as frechet_groups takes it, groups of any size >= 1; at most CLASS_GROUPS_MAX_COLUMNS columns).  Nothing
    waits for the device: returns (rec, h, check) with rec the f64 device tensor [B, 4] of { mean of h over the group's rows,
    m = sum pbar log pbar, log IS = mean h - m, non-finite rows } records (the first three NaN where the fourth is not 0), h
    the f64 device tensor [n_total] of h = sum p log p per list position (None unless return_rows; NaN for a non-finite
    row), and check() the one host read of the workspace's flag word, which raises ValueError for an index outside [0, N).
    All arithmetic is f64: float32 rows and their float64 copies give the same bits, and so do two calls."""
    check_score_rows(rows, "rows", CLASS_GROUPS_MAX_COLUMNS)
    offs, b, host_offs = _group_offsets(offsets)
    if order is None and offs[-1] > rows.shape[0]:
        raise ValueError(f"no index list: offsets name {offs[-1]} stored rows, rows holds {rows.shape[0]}")
    rows, ld, kind = _rows(rows, "rows", is_f64(rows))
    n, c = rows.shape
    dev = rows.device
    idx = _group_index(order, offs[-1], rows)
    rec = torch.empty((b, 4), dtype=torch.float64, device=dev)
    h = torch.empty(offs[-1], dtype=torch.float64, device=dev) if return_rows else None
    ws = _run("am_class_groups_" + kind, dev, "am_class_groups_workspace_bytes", (offs[-1], b, c), _ptr(rows), n, ld, c, _opt(idx),
              _host(host_offs), b, _ptr(rec), _opt(h))
    return rec, h, _index_check(ws, idx, n, "group rows")


def check_row_pair(a, b, mode, eps):
    """Everything row_pair_scores checks, without a device call; returns eps as a float."""
    if mode not in PAIR_MODES:
        raise ValueError(f"mode={mode!r} must be one of {sorted(PAIR_MODES)}")
    try:
        eps = float(eps)
    except (TypeError, ValueError):
        raise ValueError(f"eps={eps!r} must be a finite number >= 0") from None
    if not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError(f"eps={eps!r} must be a finite number >= 0")
    check_score_rows(a, "a", ROW_PAIRS_MAX_COLUMNS)
    check_score_rows(b, "b", ROW_PAIRS_MAX_COLUMNS)
    if a.dtype != b.dtype:
        raise NotImplementedError(f"the two sides must have one dtype, got {a.dtype} and {b.dtype} (convert one of them)")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"the rows are paired one to one: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    return eps


def row_pair_scores(a, b, mode, eps=0.0, return_rows=False):
    """One value per row pair (a_i, b_i) of two matrices of equal shape and dtype (am_row_pairs_f32 / _f64): mode "cosine",
    or "kl_softmax" / "kl_sigmoid" / "kl_bernoulli" with a the candidate's logits and b the reference's (eps >= 0 is added
    inside the candidate's logarithm).  Returns (sums, rows): sums the f64 device tensor [4] = { sum v, sum v^2, finite rows,
    non-finite rows } (a value that is not finite is counted and left out of the sums), rows the f64 device tensor [N] of the
    values, or None unless return_rows.  Stream-ordered, nothing waits for the device; all arithmetic is f64 and every sum
    has a fixed order."""
    eps = check_row_pair(a, b, mode, eps)
    f64 = is_f64(a)
    same = a is b
    a, lda, kind = _rows(a, "a", f64)
    b, ldb = (a, lda) if same else _rows(b, "b", f64)[:2]
    dev = _same_device(a, b)
    n, c = a.shape
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    rows = torch.empty(n, dtype=torch.float64, device=dev) if return_rows else None
    _run("am_row_pairs_" + kind, dev, "am_row_pairs_workspace_bytes", (n,), _ptr(a), lda, _ptr(b), ldb, n, c, PAIR_MODES[mode], eps,
         _opt(rows), _ptr(sums))
    return sums, rows


# ---- partitioned symmetric k-NN (multi-GPU, every rank holds the full set) ----
def knn_path(n, m, d, k, self_distance=True):
    """0 exact general kernel, 1 exact symmetric kernel, 2 / 3 f16 filter + exact verification (128 / 256-row engine)."""
    return int(_lib.load().am_knn_path(int(n), int(m), int(d), int(k), 1 if self_distance else 0))


def prdc_path(n_ref, n_cand, d):
    """0 exact kernel, 2 / 3 f16 filter + exact verification (128 / 256-row engine)."""
    return int(_lib.load().am_prdc_path(int(n_ref), int(n_cand), int(d)))


KD_TILE, KD_TILE_TAIL, KD_GENERIC, KD_SPLIT = 0, 1, 2, 3


def kd_path(n1, ldx, n2, ldy, d, m, degree=3, rbf=False):
    """Form of the float32 kernel distance for a shape (am_kd_path): 0 f32 tile kernel, 1 the same with an inner-dimension
    tail, 2 generic pointer form (a matrix of >= 4 GiB), 3 split-f16 form; -1 for shapes the entry points reject."""
    return int(_lib.load().am_kd_path(int(n1), int(ldx), int(n2), int(ldy), int(d), int(m), int(degree), 1 if rbf else 0))


def filter_engine(d):
    """Tile engine of the path-3 filter kernels for rows of d elements: 1 operand-stationary (pstat, D <= 512), 2 the same as two
    256-thread workgroups per CU (pstat64, D <= 128), 0 streamed (wide)."""
    return int(_lib.load().am_filter_engine(int(d)))


def knn_sym_eligible(n, d, k, dtype=None):
    """The partitioned symmetric sweep is a float32 form (float64 sets: row shards through knn_radii)."""
    if dtype == torch.float64:
        return False
    return bool(_lib.load().am_knn_sym_eligible(int(n), int(d), int(k)))


def knn_bounds(x_full, k, row0, nrows, prepared=None):
    """Squared upper bounds for rows [row0, row0+nrows) of the full set (column-sample pre-pass)."""
    x = as_matrix(x_full)
    n, d = x.shape
    out = torch.empty(int(nrows), dtype=torch.float32, device=x.device)
    query, tail = ("am_knn_part_workspace_bytes", (n, d, int(k))), (int(k), int(row0), int(nrows), _ptr(out))
    if prepared is not None:
        ps = prepared.struct()
        _run("am_knn_bounds_prepared_f32", x.device, *query, _ptr(x), n, _ld(x), d, ctypes.byref(ps), *tail)
    else:
        _run("am_knn_bounds_f32", x.device, *query, _ptr(x), n, _ld(x), d, *tail)
    return out


def knn_sym_part(x_full, k, part, nparts, bounds_sq, prepared=None):
    """This rank's share of the symmetric k-NN: [N, width] smallest entries per row (+inf padded)."""
    x = as_matrix(x_full)
    n, d = x.shape
    width = _lib.load().am_knn_list_width(int(k))
    bounds_sq = bounds_sq.to(torch.float32).contiguous().clone()
    out = torch.empty((n, width), dtype=torch.float32, device=x.device)
    query, tail = ("am_knn_part_workspace_bytes", (n, d, int(k))), (int(k), int(part), int(nparts), _ptr(bounds_sq), _ptr(out))
    if prepared is not None:
        ps = prepared.struct()
        _run("am_knn_sym_part_prepared_f32", x.device, *query, _ptr(x), n, _ld(x), d, ctypes.byref(ps), *tail)
    else:
        _run("am_knn_sym_part_f32", x.device, *query, _ptr(x), n, _ld(x), d, *tail)
    return out


def knn_lists_finish(lists, x_full, k):
    """[nparts, N, width] per-rank lists -> radii f32[N] (bit-identical to knn_radii(x_full, k))."""
    x = as_matrix(x_full)
    n, d = x.shape
    lists = lists.to(torch.float32).contiguous()
    nparts = lists.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    _run("am_knn_lists_finish_f32", x.device, "am_knn_lists_finish_workspace_bytes", (n, d, int(k)), _ptr(lists), nparts, _ptr(x), n,
         _ld(x), d, int(k), _ptr(out))
    return out


def prdc_counts(ref, cand, r_ref, r_cand, want_min=False, prepared_ref=None, prepared_cand=None):
    """col_count i32[Nc], row_any u8[Nr], row_cover u8[Nr] (prdc.py:34-48); with want_min=True also the row
    minimum f32[Nr] (not needed by any metric; costs extra).  float64 rows (either set): distances, radii and the comparisons
    in f64 (am_prdc_counts_f64; the row minimum is then f64 too)."""
    _require_cuda(r_ref, "r_ref")
    _require_cuda(r_cand, "r_cand")
    f64 = _any_f64(ref, cand)
    (ref, ldr, kind), (cand, ldc, _) = _rows(ref, "reference", f64), _rows(cand, "candidate", f64)
    r_ref, r_cand = r_ref.to(ref.dtype).contiguous(), r_cand.to(ref.dtype).contiguous()
    nr, d = ref.shape
    nc = cand.shape[0]
    if r_ref.numel() != nr or r_cand.numel() != nc or cand.shape[1] != d:
        raise ValueError("radius / embedding shapes do not match")
    dev = ref.device
    col = torch.empty(nc, dtype=torch.int32, device=dev)
    rany = torch.empty(nr, dtype=torch.uint8, device=dev)
    rcov = torch.empty(nr, dtype=torch.uint8, device=dev)
    rmin = torch.empty(nr, dtype=ref.dtype, device=dev) if want_min else None
    query, tail = (_query("prdc", f64), (nr, nc, d)), (d, _ptr(r_ref), _ptr(r_cand), _ptr(col), _ptr(rany), _ptr(rcov), _opt(rmin))
    if not f64 and prepared_ref is not None and prepared_cand is not None:
        pr, pc = prepared_ref.struct(), prepared_cand.struct()
        _run("am_prdc_counts_prepared_f32", dev, *query, _ptr(ref), nr, ldr, ctypes.byref(pr), _ptr(cand), nc, ldc, ctypes.byref(pc),
             *tail)
    else:
        _run("am_prdc_counts_" + kind, dev, *query, _ptr(ref), nr, ldr, _ptr(cand), nc, ldc, *tail)
    return (col, rany, rcov, rmin) if want_min else (col, rany, rcov)


def prdc_reduce(col, rany, rcov):
    """Four integer totals as a device int64[4]:
    (#cols with count>0, #rows with any, sum of counts, #rows covered)."""
    lib = _lib.load()
    for t, name in ((col, "col_count"), (rany, "row_any"), (rcov, "row_cover")):
        _require_cuda(t, name)                 # (empty row arrays are allowed: column totals only)
    # the C ABI takes raw pointers: hand it exactly the element types it reads
    col = col.to(torch.int32).contiguous()
    rany = rany.to(torch.uint8).contiguous()
    rcov = rcov.to(torch.uint8).contiguous()
    if rcov.numel() != rany.numel():
        raise ValueError("row_any / row_cover lengths differ")
    out = torch.empty(4, dtype=torch.int64, device=col.device)
    _call(lib, "am_prdc_reduce", col.device, _ptr(col), col.numel(), _ptr(rany), _ptr(rcov), rany.numel(), _ptr(out))
    return out


# ------------------------------------------------------------------ one call = one evaluate()
EVAL_FAD, EVAL_KD, EVAL_PRDC, EVAL_HEAD = 1, 2, 4, 16
_EVAL_WS = {}


def _eval_workspace(nbytes, device):
    """The evaluate workspace is kept per device and grown on demand: its size is a function of the shapes, an evaluate
    runs start to finish on one stream, and re-allocating ~1 GB per call costs the allocator round trips this entry point
    exists to avoid."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _EVAL_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        _EVAL_WS.pop(key, None)                                  # (the old block goes back to the allocator first)
        ws = None
        ws = _EVAL_WS[key] = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    return ws


def release_workspaces(device=None):
    """Hand the cached evaluate workspaces (1.2 GB per (device, stream) at 2 x 100k x 512, 19.6 GB at 2 x 1M) back to
    torch's caching allocator - for callers that run one large evaluate and then need the memory for something else.
    The next evaluate allocates again.  `device`: only that GPU's."""
    index = None if device is None else torch.device(device).index
    for key in [k for k in _EVAL_WS if index is None or k[0] == index]:
        del _EVAL_WS[key]


def _eval_request(what, idx_cand, idx_ref):
    """The request half of both evaluate calls: (flags of `what`, the two KD index tables as the library takes them, S, m)."""
    flags = sum(bit for name, bit in (("fad", EVAL_FAD), ("kd", EVAL_KD), ("prdc", EVAL_PRDC)) if name in what)
    s = m = 0
    if flags & EVAL_KD:
        idx_cand, idx_ref = _index_table(idx_cand, "idx_cand"), _index_table(idx_ref, "idx_ref")
        s, m = idx_cand.shape
    return flags, idx_cand, idx_ref, s, m


def evaluate(ref, cand, what, nearest_k=5, idx_cand=None, idx_ref=None, gamma=None, coef0=1.0, degree=3,
             given_ref=None, given_cand=None):
    """am_evaluate_f32: FAD / KD / PRDC of (candidate vs reference) as ONE stream-ordered chain with ONE read-back.
    `what`: iterable of "fad", "kd", "prdc".  given_*: dict with any of mean, cov, radii (already computed: used as they
    are) and mean_out, cov_out, radii_out (device tensors the chain writes its own results to, so that the caller keeps
    them).  Returns the raw host record: (head f64[16], mmds f64[S] or None)."""
    lib = _lib.load()
    if is_f64(ref) or is_f64(cand):
        raise ValueError("am_evaluate_f32 is the float32 chain; float64 sets run entry point by entry point (evaluate_sharded)")
    ref, cand = as_matrix(ref, "reference"), as_matrix(cand, "candidate")
    dev = _same_device(ref, cand)
    n_ref, d = ref.shape
    n_cand = cand.shape[0]
    if cand.shape[1] != d:
        raise ValueError("feature dimensions differ")
    flags, idx_cand, idx_ref, s, m = _eval_request(what, idx_cand, idx_ref)
    keep = []

    def side(given, rows):
        # the C ABI reads and writes raw pointers: every tensor is checked against the shape the chain assumes for it
        if not given:
            return None
        st = _lib.EvaluateSideStruct()
        for key in ("mean", "cov", "mean_out", "cov_out"):
            t = given.get(key)
            if t is not None:
                want = (d,) if key.startswith("mean") else (d, d)
                if tuple(t.shape) != want:
                    raise ValueError(f"{key} has shape {tuple(t.shape)}, the embeddings need {want}")
                if key.endswith("_out") and (t.dtype != torch.float64 or not t.is_contiguous()):
                    raise ValueError(f"{key} must be a contiguous f64 tensor (the chain writes into it)")
                t = _f64(t, key)
                if t.device != dev:
                    raise ValueError(f"{key} lives on {t.device}, the embeddings on {dev}")
                keep.append(t)
                setattr(st, key, t.data_ptr())
        for key in ("radii", "radii_out"):
            t = given.get(key)
            if t is not None:
                _require_cuda(t, key)
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                    raise ValueError(f"{key} must be a contiguous f32 tensor on {dev}")
                if t.numel() != rows:
                    raise ValueError(f"radius / embedding shapes do not match: {key} holds {t.numel()} values, the set {rows} rows")
                keep.append(t)
                setattr(st, key, t.data_ptr())
        return st

    s_ref, s_cand = side(given_ref, n_ref), side(given_cand, n_cand)
    with torch.cuda.device(dev):
        main = torch.cuda.current_stream(dev)
        side_stream = _side_stream(("fad", dev.index), dev)
        nb = lib.am_evaluate_workspace_bytes(n_ref, n_cand, d, int(nearest_k), s, m, flags)
        ws = _eval_workspace(nb, dev)
        out = torch.empty(EVAL_HEAD + s, dtype=torch.float64, device=dev)
        timer = KernelTimer.active
        if timer is not None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(main)
        status = lib.am_evaluate_f32(_ptr(ref), n_ref, _ld(ref), _ptr(cand), n_cand, _ld(cand), d, flags, int(nearest_k),
                                     _ptr(idx_cand) if s else None, _ptr(idx_ref) if s else None, s, m,
                                     float(1.0 / d if gamma is None else gamma), float(coef0), int(degree),
                                     ctypes.byref(s_ref) if s_ref is not None else None,
                                     ctypes.byref(s_cand) if s_cand is not None else None, _ptr(out), _ptr(ws), nb,
                                     ctypes.c_void_p(main.cuda_stream), ctypes.c_void_p(side_stream.cuda_stream))
        if timer is not None:
            b.record(main)
            timer.records.append(("am_evaluate_f32", a, b))
        _lib.check(status, "am_evaluate_f32")
        for t in (ref, cand, *keep):
            t.record_stream(side_stream)
        host = out.cpu()                                             # the one read-back
    head = host[:EVAL_HEAD].tolist()
    return head, (host[EVAL_HEAD:].numpy() if s else None)


def evaluate_sharded_c(ref_local, cand_local, ref_counts, cand_counts, what, coll, nearest_k=5, idx_cand=None, idx_ref=None,
                       gamma=None, coef0=1.0, degree=3, overlap=True):
    """am_evaluate_sharded_f32: this rank's share of a row-sharded evaluate as ONE library call - the exchange schedule of
    distributed.evaluate_sharded behind the C ABI, with the collectives supplied as hooks (`coll`: collectives.TorchCollectives
    here, am_rccl_collectives for a host that is not Python).  ref_counts / cand_counts: rows of every rank.  overlap=False
    issues the collectives on the compute stream.  Returns the host record like evaluate(): (head f64[16], mmds or None)."""
    lib = _lib.load()
    if is_f64(ref_local) or is_f64(cand_local):
        raise ValueError("am_evaluate_sharded_f32 is the float32 schedule")
    rank, world = coll.rank, coll.world
    ref_counts, cand_counts = [int(c) for c in ref_counts], [int(c) for c in cand_counts]
    if len(ref_counts) != world or len(cand_counts) != world:
        raise ValueError("one shard size per rank")
    ref_local, cand_local = as_matrix(ref_local, "reference"), as_matrix(cand_local, "candidate")
    dev = _same_device(ref_local, cand_local)
    d = ref_local.shape[1]
    if cand_local.shape[1] != d or ref_local.shape[0] != ref_counts[rank] or cand_local.shape[0] != cand_counts[rank]:
        raise ValueError("the shards do not match the shard sizes / each other")
    flags, idx_cand, idx_ref, s, m = _eval_request(what, idx_cand, idx_ref)
    rc_arr = (ctypes.c_int64 * world)(*ref_counts)
    cc_arr = (ctypes.c_int64 * world)(*cand_counts)
    with torch.cuda.device(dev):
        main = torch.cuda.current_stream(dev)
        side_stream = _side_stream(("fad", dev.index), dev)
        comm_stream = _side_stream(("comm", dev.index), dev)
        nb = lib.am_evaluate_sharded_workspace_bytes(rc_arr, cc_arr, rank, world, d, int(nearest_k), s, m, flags)
        if nb == 0:
            raise ValueError(f"empty embedding set: {sum(ref_counts)} reference and {sum(cand_counts)} candidate rows over {world} ranks")
        ws = coll.expose(_eval_workspace(nb, dev))            # (kept per device and stream, like the fused call's)
        out = torch.empty(EVAL_HEAD + s, dtype=torch.float64, device=dev)
        status = lib.am_evaluate_sharded_f32(
            _ptr(ref_local) if ref_counts[rank] else None, _ld(ref_local), _ptr(cand_local) if cand_counts[rank] else None,
            _ld(cand_local), d, rc_arr, cc_arr, coll.byref(), flags, int(nearest_k), _ptr(idx_cand) if s else None,
            _ptr(idx_ref) if s else None, s, m, float(1.0 / d if gamma is None else gamma), float(coef0), int(degree), _ptr(out),
            _ptr(ws), nb, ctypes.c_void_p(main.cuda_stream), ctypes.c_void_p(side_stream.cuda_stream),
            ctypes.c_void_p(comm_stream.cuda_stream if overlap else main.cuda_stream))
        if getattr(coll, "error", None) is not None:
            raise coll.error
        _lib.check(status, "am_evaluate_sharded_f32")
        for t in (ref_local, cand_local):
            t.record_stream(side_stream)
            t.record_stream(comm_stream)
        host = out.cpu()                                     # the one read-back: the pack kernel behind it waits for all three streams' work
    head = host[:EVAL_HEAD].tolist()
    return head, (host[EVAL_HEAD:].numpy() if s else None)
