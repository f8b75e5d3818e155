"""Shared by tests/test_metrics.py and tests/test_gpu_metrics_shapes.py: inputs for the first-generation
metric kernels of sd_metrics.hip (k_pairwise, k_ade_fde, k_segment_mean) at ragged shapes, with float64
references from the oracle (oracle.metric_lat_apd / metric_apd / metric_ade / metric_mmade).  CPU only.
Every case is built once per session (lru_cache) and never modified.

Exact tier.  Integer-valued float32 inputs, so that every float32 partial sum on the device is an exact
integer below 2^24 and only the last steps round:
  pairwise  values in [-8, 8]: a pair's L1 sum is at most 16 X and its sum of squares at most 256 X
            (X <= 459: 117504 < 2^24).  What rounds: one sqrtf per pair (<= 1 ulp), the float64 sum (nothing
            visible), one division and one cast (1/2 ulp each): 2 ulp, doubled for slack -> PAIR_ULPS = 4.
  sweep     sample i = base + c_i e_f: every pair distance is |c_i - c_j| in L1 and in L2, so a dropped or
            double-counted feature position f moves the answer by an integer.
  ade/fde   pred[s, t] = target[t] + m(s, t) e_f(s, t): a frame's distance is exactly m, a sample's frame sum an
            exact integer, only `/ T` rounds (1/2 ulp; the oracle's float64 quotient cast to float32 may
            differ from it by one more) -> ADE_ULPS = 2.
  mm        pred[i, s, t] = base[i, t] + m e_f, gt[i, j, t] = base[i, t] - n e_f on the same axis f = f(i, t):
            the frame distance is m + n.  k_segment_mean adds at most 70 such float32 values in sequence and
            divides once: (count + 2) 2^-24 relative.

Bounded tier.  Normal inputs at the same shapes.  All summed terms are non-negative, so a sequential float32
sum of n terms has a relative error of at most n u (u = 2^-24, first order):
  pairwise  64 fma steps inside a chunk, one add per chunk, the square root and the final division / cast:
            (64 + ceil(X / 64) + 2) u
  ade       the lane's chain of ceil(F / 64) fma steps, six butterfly adds, the square root, T frame adds
            and one division: (T + ceil(F / 64) + 8) u;  fde: (ceil(F / 64) + 8) u
"""
import collections
import functools

import torch

import oracle as O
from skeletondiffusion_amd import synthetic

U = 2.0 ** -24    # unit roundoff of float32
ULP = 2.0 ** -23  # one unit in the last place, relative
PAIR_ULPS, ADE_ULPS = 4, 2
B = 3             # sequences per case unless a case says otherwise
LIMIT = 2 ** 24   # integers below it are exact in float32
CHUNK = 64        # sd_metrics.hip kChunk, and the lanes of a wave in k_ade_fde

# ---- shapes -----------------------------------------------------------------------------------------------------
PAIR_S = (2, 3, 23, 24, 64)      # 23 -> 253 pairs, 24 -> 276: either side of k_pairwise's 256 first pair slots
PAIR_X = (1, 63, 64, 65, 459)    # 459 = 3 * 153: seven full chunks and 11
PAIR_SHAPES = [(S, X) for S in PAIR_S for X in PAIR_X]
SWEEP_S, SWEEP_X = 5, 459
SWEEP_POSITIONS = (0, 63, 64, 127, 128, 448, 458)
SWEEP_COEFFS = (-3, 0, 1, 5, 9)  # distinct

ADE_S = (1, 3, 4, 5, 64)         # k_ade_fde's waves take samples s, s + 4, ...
ADE_T = (1, 2, 7)
ADE_F = (1, 48, 63, 64, 65, 153, 156, 193)
ADE_KEEP = ((5, 7, 153), (64, 7, 193))
ADE_SHAPES = [(S, T, F) for i, S in enumerate(ADE_S) for j, T in enumerate(ADE_T) for k, F in enumerate(ADE_F)
              if (i + j + k) % 3 == 0 or (S, T, F) in ADE_KEEP]
ADE_MARKS = (0, 63, 64, 127, 128)  # and F - 1

MM_SEQ, MM_S, MM_T, MM_F = 300, 3, 2, 5
MM_COUNTS = (1, 2, 5)
MM_LONG = (257, 70)              # sequence 257 (k_segment_mean's second block) has 70 ground truths

MANO_SHAPE, MANO_T0, MANO_T = (2, 50, 8, 51, 3), 2, 7
DTYPES = (torch.float64, torch.float16, torch.bfloat16)
STRUCT_B, STRUCT_S, STRUCT_T, STRUCT_X = 5, 3, 3, 65
NF_S, NF_T, NF_F, NF_SEQ = 5, 3, 65, 1
NF_SAMPLES = (0, 2, 4)           # first, middle, last
NF_COUNTS = (2, 1, 3)


def ceil_div(a, b):
    return -(-a // b)


def pairwise_bound(X):
    return (CHUNK + ceil_div(X, CHUNK) + 2) * U


def ade_bound(T, F):
    return (T + ceil_div(F, CHUNK) + 8) * U


def fde_bound(F):
    return (ceil_div(F, CHUNK) + 8) * U


def mm_bound(count):
    return (count + 2) * U


def rel_err(got, ref):
    """max |got - ref| / |ref| in float64; where ref is 0, got must be 0 too (else inf)"""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    rel = torch.where(ref != 0, err / ref.abs().clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
    return float(rel.max())


def _gen(*key):
    seed = 977
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _ints(shape, g, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# ---- pairwise ---------------------------------------------------------------------------------------------------
Pairwise = collections.namedtuple("Pairwise", ["x", "lat_apd", "apd"])


def _pairwise(x):
    return Pairwise(x, O.metric_lat_apd(x), O.metric_apd(x.unsqueeze(2)))


@functools.lru_cache(maxsize=None)
def pairwise_exact(S, X):
    """x (B, S, X) integer-valued in [-8, 8] and the oracle's lat_apd / apd"""
    return _pairwise(_ints((B, S, X), _gen(1, S, X)))


@functools.lru_cache(maxsize=None)
def pairwise_normal(S, X):
    return _pairwise(torch.randn((B, S, X), generator=_gen(2, S, X)))


def pair_sums(x):
    """Per sequence and pair i < j the integer L1 sum and sum of squares (int64, (B, P)) of integer-valued x"""
    xi = x.to(torch.int64)
    S = x.shape[1]
    iu = torch.triu_indices(S, S, offset=1)
    d = xi[:, iu[0]] - xi[:, iu[1]]
    return d.abs().sum(-1), (d * d).sum(-1)


@functools.lru_cache(maxsize=None)
def pairwise_sweep():
    """(Pairwise of x (len(SWEEP_POSITIONS), SWEEP_S, SWEEP_X), expected (sequences,) float64): sequence q differs
    between its samples at feature SWEEP_POSITIONS[q] alone, by SWEEP_COEFFS in an order that turns with q"""
    n = len(SWEEP_POSITIONS)
    x = _ints((n, 1, SWEEP_X), _gen(3)).repeat(1, SWEEP_S, 1)
    c = torch.tensor(SWEEP_COEFFS, dtype=torch.float64)
    for q, f in enumerate(SWEEP_POSITIONS):
        x[q, :, f] += torch.roll(c, q).float()
    iu = torch.triu_indices(SWEEP_S, SWEEP_S, offset=1)
    want = (c[iu[0]] - c[iu[1]]).abs().mean()  # the same for every order of the coefficients
    return _pairwise(x), want.repeat(n)


# ---- ade / fde --------------------------------------------------------------------------------------------------
AdeCase = collections.namedtuple("AdeCase", ["target", "pred", "m", "f", "ade", "fde", "ade_none", "fde_none"])


def _ade(target, pred, m=None, f=None):
    return AdeCase(target, pred, m, f, O.metric_ade(target, pred), O.metric_ade(target, pred, last_only=True),
                   O.metric_ade(target, pred, reduction="none"),
                   O.metric_ade(target, pred, reduction="none", last_only=True))


def ade_marks(F):
    """The feature positions a frame's difference is put at: the ends of k_ade_fde's lane passes, and F - 1"""
    return sorted({p for p in ADE_MARKS + (F - 1,) if p < F})


def ade_weights(S, T):
    """m (B, S, T) int64 in 1..7.  Sequence b's FDE minimum is sample d = (S - 1 - b) % S (last frame 1, earlier
    frames 7) and, for S, T >= 2, its ADE minimum sample a = (d + 1) % S (earlier frames 1, last frame 4: frame
    sum T + 3, below the 3 T of any other sample and the 7 T - 6 of d).  b = 0: the FDE minimum is the last
    sample; b = 1: the ADE minimum is."""
    b, s, t = torch.meshgrid(torch.arange(B), torch.arange(S), torch.arange(T), indexing="ij")
    m = 3 + (5 * b + 7 * s + 3 * t) % 5
    for q in range(B):
        d = (S - 1 - q) % S
        if S > 1:
            a = (d + 1) % S
            m[q, a, :] = 1
            m[q, a, T - 1] = 4
        m[q, d, :] = 7
        m[q, d, T - 1] = 1
    return m


def ade_positions(S, T, F):
    """f (B, S, T) int64: the frames of the case, counted through sequences, samples and frames, walk ade_marks(F)
    so that the case's very last frame (last sequence, last sample, last frame) differs at F - 1"""
    marks = torch.tensor(ade_marks(F))
    k = torch.arange(B * S * T)
    return marks[(k + len(marks) - 1 - (B * S * T - 1)) % len(marks)].reshape(B, S, T)


@functools.lru_cache(maxsize=None)
def ade_exact(S, T, F):
    target = _ints((B, T, F), _gen(4, S, T, F))
    m, f = ade_weights(S, T), ade_positions(S, T, F)
    pred = target[:, None].repeat(1, S, 1, 1)
    pred.scatter_add_(3, f[..., None], m[..., None].float())
    return _ade(target, pred, m, f)


def ade_by_hand(m):
    """(ade_none, fde_none, ade, fde) in float64 from the frame distances m (B, S, T)"""
    per = m.double().sum(-1) / m.shape[-1]
    last = m[..., -1].double()
    return per, last, per.min(-1).values, last.min(-1).values


@functools.lru_cache(maxsize=None)
def ade_normal(S, T, F):
    g = _gen(5, S, T, F)
    target = torch.randn((B, T, F), generator=g)
    return _ade(target, target[:, None] + 0.5 * torch.randn((B, S, T, F), generator=g))


# ---- mmade / mmfde ----------------------------------------------------------------------------------------------
MMCase = collections.namedtuple("MMCase", ["pred", "mm_gt", "counts", "m", "n", "mmade", "mmfde", "futures",
                                           "row_ptr", "col", "segment_idx"])


def mm_counts():
    counts = [MM_COUNTS[i % len(MM_COUNTS)] for i in range(MM_SEQ)]
    counts[MM_LONG[0]] = MM_LONG[1]
    return counts


@functools.lru_cache(maxsize=None)
def mm_exact():
    """MM_SEQ sequences; `futures` holds every ground truth, sequence i's at rows segment_idx[i] .. + counts[i],
    and (row_ptr, col) is the adjacency that gives each of those rows that same set (MultimodalGT)."""
    g = _gen(6)
    counts = mm_counts()
    base = _ints((MM_SEQ, MM_T, MM_F), g)
    m = torch.randint(1, 6, (MM_SEQ, MM_S, MM_T), generator=g)
    i, t = torch.meshgrid(torch.arange(MM_SEQ), torch.arange(MM_T), indexing="ij")
    f = (i + 2 * t) % MM_F
    pred = base[:, None].repeat(1, MM_S, 1, 1)
    pred.scatter_add_(3, f[:, None, :, None].expand(MM_SEQ, MM_S, MM_T, 1), m[..., None].float())
    mm_gt, n = [], []
    for q, c in enumerate(counts):
        nq = torch.randint(0, 5, (c, MM_T), generator=g)
        gt = base[q][None].repeat(c, 1, 1)
        gt.scatter_add_(2, f[q][None, :, None].expand(c, MM_T, 1), -nq[..., None].float())
        mm_gt.append(gt)
        n.append(nq)
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    row_ptr, col = [0], []
    for q, c in enumerate(counts):
        for _ in range(c):
            col += list(range(off[q], off[q + 1]))
            row_ptr.append(len(col))
    return MMCase(pred, mm_gt, counts, m, n, O.metric_mmade(pred, mm_gt), O.metric_mmade(pred, mm_gt, last_only=True),
                  torch.cat(mm_gt), torch.tensor(row_ptr), torch.tensor(col), off[:-1])


def mm_by_hand(m, n):
    """(mmade, mmfde) in float64: the frame distance of sample s to ground truth j is m[s, t] + n[j, t]"""
    ade, fde = [], []
    for mq, nq in zip(m, n):
        d = (mq[None, :, :] + nq[:, None, :]).double()  # (count, S, T)
        ade.append((d.sum(-1) / d.shape[-1]).min(-1).values.mean())
        fde.append(d[..., -1].min(-1).values.mean())
    return torch.stack(ade), torch.stack(fde)


# ---- bounded tier: the MANO rows, a permuted view, other input types --------------------------------------------
@functools.lru_cache(maxsize=None)
def mano_case():
    """pred (2, 50, 8, 51, 3), target (2, 8, 51, 3) for apd / ade / fde with t0 = 2, t = 7: frames of F = 153, and a
    time slice that is not contiguous.  -> (target, pred, apd, ade, fde) with the oracle's values of the slice"""
    target = torch.from_numpy(synthetic.normal(MANO_SHAPE[:1] + MANO_SHAPE[2:], seed=51))
    pred = target[:, None] + 0.5 * torch.from_numpy(synthetic.normal(MANO_SHAPE, seed=52))
    return (target, pred, O.metric_apd(pred, MANO_T0, MANO_T), O.metric_ade(target, pred, MANO_T0, MANO_T),
            O.metric_ade(target, pred, MANO_T0, MANO_T, last_only=True))


PERM_S, PERM_T, PERM_F = 5, 7, 65


@functools.lru_cache(maxsize=None)
def permuted_case():
    """`stored` (B, T, S, F): its view stored.permute(0, 2, 1, 3) is the pred (B, S, T, F) of an AdeCase, and
    flattened to (B, S, T F) the x of a Pairwise"""
    c = ade_normal(PERM_S, PERM_T, PERM_F)
    stored = c.pred.permute(0, 2, 1, 3).contiguous()
    assert not stored.permute(0, 2, 1, 3).is_contiguous()
    return stored, c, _pairwise(c.pred.reshape(B, PERM_S, PERM_T * PERM_F))


@functools.lru_cache(maxsize=None)
def dtype_case(dtype):
    """(target, pred) in `dtype` at (S, T, F) = (5, 2, 153); the AdeCase and Pairwise of their float32 casts: the
    wrappers cast to float32, so that is the input the oracle gets"""
    g = _gen(7, DTYPES.index(dtype))
    target = torch.randn((B, 2, 153), generator=g, dtype=torch.float64).to(dtype)
    pred = (target.double()[:, None] + 0.5 * torch.randn((B, 5, 2, 153), generator=g, dtype=torch.float64)).to(dtype)
    return target, pred, _ade(target.float(), pred.float()), _pairwise(pred.float().reshape(B, 5, 306))


# ---- structure and non-finite tiers -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def structure_case():
    """(x (5, 3, 65), target (5, 3, 65), pred (5, 3, 3, 65)): odd sizes, so that the sequences' first elements fall
    on every 4-byte phase of a 16-byte line"""
    g = _gen(8)
    x = torch.randn((STRUCT_B, STRUCT_S, STRUCT_X), generator=g)
    target = torch.randn((STRUCT_B, STRUCT_T, STRUCT_X), generator=g)
    return x, target, target[:, None] + 0.5 * torch.randn((STRUCT_B, STRUCT_S, STRUCT_T, STRUCT_X), generator=g)


@functools.lru_cache(maxsize=None)
def nonfinite_clean():
    """(target (B, T, F), pred (B, S, T, F), mm_gt list with NF_COUNTS ground truths) before a value is planted"""
    g = _gen(9)
    target = torch.randn((B, NF_T, NF_F), generator=g)
    pred = target[:, None] + 0.5 * torch.randn((B, NF_S, NF_T, NF_F), generator=g)
    mm_gt = [target[q][None] + 0.3 * torch.randn((c, NF_T, NF_F), generator=g) for q, c in enumerate(NF_COUNTS)]
    return target, pred, mm_gt


def planted(samples, value):
    """nonfinite_clean's pred with `value` in the last feature of the last frame (the second pass of lane 0, seen
    by fde as well as ade) of each of `samples` of sequence NF_SEQ"""
    pred = nonfinite_clean()[1].clone()
    for k in samples:
        pred[NF_SEQ, k, NF_T - 1, NF_F - 1] = value
    return pred


NonFinite = collections.namedtuple("NonFinite", ["pred", "ade", "fde", "ade_none", "fde_none", "mmade", "mmfde",
                                                 "lat_apd", "apd"])


@functools.lru_cache(maxsize=None)
def nonfinite_case(samples, value):
    """The oracle's values (torch.min and mean on float64 CPU tensors) with `value` planted in `samples`"""
    target, _, mm_gt = nonfinite_clean()
    pred = planted(samples, value)
    c = _ade(target, pred)
    return NonFinite(pred, c.ade, c.fde, c.ade_none, c.fde_none, O.metric_mmade(pred, mm_gt),
                     O.metric_mmade(pred, mm_gt, last_only=True), O.metric_lat_apd(pred), O.metric_apd(pred))


def bounded_shapes():
    """Every (kernel, bound) of the bounded tier, for the check that none is looser than 1e-5"""
    out = [("pairwise", (S, X), pairwise_bound(X)) for S, X in PAIR_SHAPES]
    for S, T, F in ADE_SHAPES + [(PERM_S, PERM_T, PERM_F), (5, 2, 153), (MANO_SHAPE[1], MANO_T - MANO_T0, 153)]:
        out += [("ade", (S, T, F), ade_bound(T, F)), ("fde", (S, T, F), fde_bound(F))]
    out += [("pairwise", (PERM_S, PERM_T * PERM_F), pairwise_bound(PERM_T * PERM_F)),
            ("pairwise", (5, 306), pairwise_bound(306)),
            ("pairwise", (MANO_SHAPE[1], (MANO_T - MANO_T0) * 153), pairwise_bound((MANO_T - MANO_T0) * 153))]
    return out
