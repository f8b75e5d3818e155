"""The multimodal ground truth on the device: which test segments start from a similar pose,
the reference's `get_multimodal_gt` (src/data/loaders/base/math_utils.py:59-110), and what hangs on it.

    cdist(x1, x2)                        exact pairwise L2 distance from differences (sd_cdist): torch.cdist(...,
                                         compute_mode='donot_use_mm_for_euclid_dist'), math_utils.py:63
    get_multimodal_gt(last_obs, thr)     the pairs with distance < thr as a CSR adjacency -> MultimodalGT
    MultimodalGT.to_dict / save / load   the reference's {segment: {similar segments}} and its mmgt_{split}.txt
                                         file (create_dataset_utils.py:46-49, :64-65), both directions
    MultimodalGT.mm_gt(futures, idx)     the per-segment (n_i, T, J, 3) tensors metrics.mmade / mmfde take
                                         (base_dataset.py:181-186)
    MultimodalGT.mmade / mmfde(pred, futures, idx)   the same metrics from device index ops, no Python lists
    MultimodalGT.gt_apd(futures)         apd (multimodal.py:15-35) of every segment's set of similar futures: the
                                         table behind the reference's shipped mmapd_GT.csv (metrics.APDEAccumulator)

Distances are computed on ROCm tensors only (no CPU path); the dict and file halves need no device.
"""
from __future__ import annotations

import ast
import json

import torch

from . import _lib, metrics
from ._lib import SkelDiffError, check


def cdist(x1: torch.Tensor, x2: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """x1 (m, D), x2 (n, D) -> (m, n) float32, dist[i, j] = sqrt(sum_k (x1[i, k] - x2[j, k])^2) summed in one
    fixed order: a value depends on the two rows only, so cdist(x, x) is bitwise symmetric with a zero diagonal
    and row chunks give the bits of one call.  Contiguous float32 views are read where they lie."""
    a, b = metrics._device_tensor(x1, "x1"), metrics._device_tensor(x2, "x2")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"cdist: (m, D) and (n, D) expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    m, n = a.shape[0], b.shape[0]
    if out is None:
        out = torch.empty(m, n, device=a.device, dtype=torch.float32)
    elif tuple(out.shape) != (m, n) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != a.device:
        raise ValueError(f"cdist: out must be a contiguous float32 ({m}, {n}) tensor on {a.device}")
    stream = torch.cuda.current_stream(a.device).cuda_stream
    check(_lib.lib().sd_cdist(a.data_ptr(), m, b.data_ptr(), n, a.shape[1], out.data_ptr(), stream))
    return out


class MultimodalGT:
    """A CSR adjacency over N segments: segment i is similar to col[row_ptr[i] : row_ptr[i + 1]] (ascending, i
    itself included, symmetric), as the reference's dict of sorted sets.  row_ptr (N + 1) and col are int64 on
    `device`; `row_ptr_host` is a host copy, so set sizes are known without a synchronisation."""

    def __init__(self, row_ptr, col, device=None):
        row_ptr, col = torch.as_tensor(row_ptr, dtype=torch.int64), torch.as_tensor(col, dtype=torch.int64)
        device = torch.device(device) if device is not None else col.device
        self.row_ptr_host = row_ptr.detach().cpu()
        if row_ptr.dim() != 1 or row_ptr.numel() < 1 or col.dim() != 1 or int(self.row_ptr_host[0]) != 0 or \
                int(self.row_ptr_host[-1]) != col.numel() or bool((self.row_ptr_host[1:] < self.row_ptr_host[:-1]).any()):
            raise ValueError("MultimodalGT: row_ptr must rise from 0 to len(col)")
        self.device = device
        self.row_ptr = row_ptr.detach().to(device).contiguous()
        self.col = col.detach().to(device).contiguous()

    def __len__(self) -> int:
        return self.row_ptr_host.numel() - 1

    # ---- the reference's dict and file ---------------------------------------------------------------------
    def to_dict(self):
        """math_utils.py:106: {segment: {similar segments}}, keys and members ascending."""
        rp, col = self.row_ptr_host.tolist(), self.col.cpu().tolist()
        return {i: set(col[rp[i]:rp[i + 1]]) for i in range(len(self))}

    @classmethod
    def from_dict(cls, d, device="cpu") -> "MultimodalGT":
        n = max(d) + 1 if d else 0
        rows = [sorted(d.get(i, ())) for i in range(n)]
        row_ptr = [0]
        for r in rows:
            row_ptr.append(row_ptr[-1] + len(r))
        return cls(row_ptr, [c for r in rows for c in r], device)

    def save(self, path) -> None:
        """create_dataset_utils.py:64-65: json.dump(str(dict))."""
        with open(path, "w") as f:
            json.dump(str(self.to_dict()), f)

    @classmethod
    def load(cls, path, device="cpu") -> "MultimodalGT":
        """create_dataset_utils.py:46-49 / base_dataset.py:146: ast.literal_eval(json.load(f))."""
        with open(path) as f:
            return cls.from_dict(ast.literal_eval(json.load(f)), device)

    # ---- the metrics' ground truths ------------------------------------------------------------------------
    def _futures(self, futures):
        if futures.shape[0] != len(self):
            raise ValueError(f"MultimodalGT: {futures.shape[0]} futures for {len(self)} segments")
        return futures

    def _host_index(self, segment_idx) -> torch.Tensor:
        """segment_idx as a host int64 tensor (a list or a host tensor costs nothing; a device tensor is copied)."""
        idx = torch.as_tensor(segment_idx, dtype=torch.int64).detach().cpu().reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError(f"MultimodalGT: segment_idx outside 0..{len(self) - 1}")
        return idx

    def mm_gt(self, futures: torch.Tensor, segment_idx):
        """base_dataset.py:181-186 per segment of the batch: the list of (n_i, T, J, 3) tensors
        `futures[similar segments of i]`, members ascending; futures (N, T, J, 3) of all segments."""
        futures = self._futures(futures)
        rp = self.row_ptr_host.tolist()
        return [futures.index_select(0, self.col[rp[i]:rp[i + 1]].to(futures.device)) for i in self._host_index(segment_idx).tolist()]

    def _mm(self, pred, futures, segment_idx, t0, t, want_ade):
        futures = self._futures(futures)
        pred = metrics._time_slice(pred, t0, t, 2)
        B, S, T = pred.shape[:3]
        idx = self._host_index(segment_idx)
        if idx.numel() != B:
            raise ValueError(f"segment_idx has {idx.numel()} entries for {B} sequences")
        p = metrics._device_tensor(pred.reshape(B, S, T, metrics._flat(pred.shape[3:])), "pred")
        dev, F = p.device, p.shape[3]
        g = metrics._time_slice(metrics._device_tensor(futures, "futures"), t0, t, 1)
        if g.shape[1] != T or metrics._flat(g.shape[2:]) != F:
            raise ValueError(f"futures frames {tuple(g.shape[1:])} do not match pred frames {tuple(pred.shape[2:])}")
        cnt_host = self.row_ptr_host[idx + 1] - self.row_ptr_host[idx]
        if B and int(cnt_host.min()) == 0:  # as metrics.mmade: the reference's reshape of an empty set raises
            raise RuntimeError("mmade/mmfde: a sequence has no multimodal ground truths")
        npairs = int(cnt_host.sum())  # host arithmetic on the host copy: no synchronisation
        idx_d, cnt = idx.to(dev), cnt_host.to(dev)
        off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(cnt, 0)
        pair_seq = torch.repeat_interleave(torch.arange(B, dtype=torch.int64, device=dev), cnt, output_size=npairs)
        member = self.row_ptr.to(dev)[idx_d][pair_seq] + (torch.arange(npairs, dtype=torch.int64, device=dev) - off[pair_seq])
        gts = g.index_select(0, self.col.to(dev)[member]).reshape(npairs, T, F)
        pair = torch.empty(max(npairs, 1), device=dev, dtype=torch.float32)
        out = torch.empty(B, device=dev, dtype=torch.float32)
        stream = torch.cuda.current_stream(dev).cuda_stream
        args = (pair, None, out, None) if want_ade else (None, pair, None, out)
        check(_lib.lib().sd_mm_ade_fde(p.data_ptr(), gts.data_ptr() if npairs else None, pair_seq.data_ptr() if npairs else None,
                                       npairs, off.data_ptr(), B, S, T, F, *(_lib.ptr(a) for a in args), stream))
        return out

    def mmade(self, pred, futures, segment_idx, t0: int = 0, t: int = -1, **kwargs) -> torch.Tensor:
        """metrics.mmade(target, pred, self.mm_gt(futures, segment_idx), t0, t), bit for bit, with the ground
        truths gathered by device index ops: pred (B, S, T, J, 3), futures (N, T, J, 3), segment_idx the B
        segment numbers of the batch (a list or host tensor: set sizes come from the host row_ptr)."""
        return self._mm(pred, futures, segment_idx, t0, t, True)

    def mmfde(self, pred, futures, segment_idx, t0: int = 0, t: int = -1, **kwargs) -> torch.Tensor:
        """As mmade, on the last frame of the slice."""
        return self._mm(pred, futures, segment_idx, t0, t, False)

    def gt_apd(self, futures: torch.Tensor, max_bytes: int = 4 << 30) -> torch.Tensor:
        """(N,) float32: per segment the reference's `apd(mm_gt_i[None])`, the mean pairwise L2 distance between
        the flattened futures of its set (0 for a set of one, NaN for an empty one): one sd_cdist over all
        futures, then sd_set_mean_distance.  The (N, N) matrix must fit `max_bytes`."""
        futures = self._futures(futures)
        N = len(self)
        if N * N * 4 > max_bytes:
            raise SkelDiffError(f"gt_apd: the distance matrix of N = {N} segments takes {N * N * 4} bytes, above the limit of "
                                f"{max_bytes} bytes (max_bytes)")
        x = metrics._device_tensor(futures.reshape(N, -1), "futures")
        dev = x.device
        dist = cdist(x, x)
        out = torch.empty(N, device=dev, dtype=torch.float32)
        row_ptr, col = self.row_ptr.to(dev), self.col.to(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(_lib.lib().sd_set_mean_distance(dist.data_ptr(), N, row_ptr.data_ptr(), _lib.ptr(col) if col.numel() else None, N,
                                              out.data_ptr(), stream))
        return out


def get_multimodal_gt(last_obs: torch.Tensor, multimodal_threshold: float, chunk_rows: int = 2048) -> MultimodalGT:
    """math_utils.py:59-110 on the device: last_obs (N, J, 3) or (N, D), the last observed pose of every segment
    in metric space (the caller applies `transform_to_metric_space`, as the reference does before :102).  Per
    chunk of rows one sd_cdist into a (chunk_rows, N) buffer -- the reference's batch size --, `d < threshold`
    (the strict comparison of :64, on the distance, not its square) and nonzero(), which reads the hit count
    (the one host read per chunk).  The distance is bitwise symmetric, so is the adjacency."""
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be >= 1")
    N = last_obs.shape[0]
    x = metrics._device_tensor(last_obs.reshape(N, -1), "last_obs")
    dev = x.device
    buf = torch.empty(min(chunk_rows, N), N, device=dev, dtype=torch.float32)
    rows, cols = [], []
    for r0 in range(0, N, chunk_rows):
        r1 = min(N, r0 + chunk_rows)
        d = cdist(x[r0:r1], x, out=buf[:r1 - r0])
        hit = (d < multimodal_threshold).nonzero()  # row-major: rows ascending, columns ascending within a row
        rows.append(hit[:, 0] + r0)
        cols.append(hit[:, 1])
    rows = torch.cat(rows) if rows else torch.empty(0, dtype=torch.int64, device=dev)
    col = torch.cat(cols) if cols else torch.empty(0, dtype=torch.int64, device=dev)
    row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    return MultimodalGT(row_ptr, col, dev)


__all__ = ["cdist", "MultimodalGT", "get_multimodal_gt"]
