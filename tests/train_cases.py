"""Shared by tests/test_training.py and tests/test_gpu_train_shapes.py: shapes and inputs for the training
graph-linear of csrc/sd_train.hip (sd_gl_train_forward / _backward) off the release Denoiser's shapes, with
float64 references.  CPU only.  Every case is built once per session (lru_cache) and never modified.

Exact mode.  x, W, bias and dy hold integers in [-2, 2] ([-1, 1] from J = 33 on) and ghat multiples of 0.5 in
[-1, 1], with negative entries and not symmetric.  Every product is then a multiple of 0.5, and so is every
partial sum of every output element in whatever order and grouping a kernel adds them, bounded in magnitude by
that element's sum of |terms|.  A multiple of 0.5 below 2^22 has at most 23 significant bits, so while the largest
sum of |terms| stays below LIMIT = 2^22 nothing rounds in float32: y, dx, dW, dbias and dghat must equal the
float64 reference bit for bit, and a masking, clamp, split or transpose error changes bits.  `exact_case` computes
that sum per output by running the same reference over the absolute values of the inputs (all terms then add up
with one sign); the tests assert it before they compare.  It is a condition on the inputs, not a measurement of
the kernels.

A case may thin x and dy (`density`, the fraction of non-zero entries): at 4,100 rows x 192 x 192 dense inputs put
dghat's sum of |terms| (rows N |dy| (K |W| |x| + |bias|), about 2.6e8) far past LIMIT; one entry in 16 keeps it
near 1.7e6 and still leaves ~200,000 non-zero entries of x and of dy spread over every split and every tile.
"""
import collections
import functools

import torch

LIMIT = 2.0 ** 22

TK = 32          # sd_train.hip: depth of a k_gemm tile (dW's kchunk is a multiple of it)
MAX_SPLITS = 32  # sd_train.hip splits_for


def splits_for(rows):
    """sd_train.hip splits_for: clamp(ceil(rows / 256), 1, 32) row ranges of the dW reduction."""
    return max(1, min(MAX_SPLITS, -(-rows // 256)))


def workspace_bytes(rows, J, K, N, n_types):
    """What sd_gl_train_workspace_bytes must hold: dz and the largest of the three partial buffers."""
    types = max(1, n_types)
    part = max(splits_for(rows) * types * N * K, -(-rows // 4) * J * J, -(-rows // 16) * types * N)
    return 4 * (rows * J * N + part)


# (J, K, N, n_types (0 = shared weights), rows): the branch each is the smallest shape for
GL_CASES = [
    (16, 3, 288, 10, 37),     # encoder W_ih: forward, dx and dW on k_gemm<false> (K = 3); k_dghat_part16
    (21, 96, 3, 13, 37),      # decoder fc: forward k_gemm<true> at N = 3 (the gnc = N - 1 clamp); dx over 3 terms and dW with M = 3 on k_gemm<false>; scalar k_dghat_part<1>; k_mix<8> at N = 3
    (1, 1, 1, 0, 1),          # everything degenerate; shared weights; J <= 16 with N % 4 != 0: k_dghat_part<1>, not k_dghat_part16
    (16, 100, 36, 10, 65),    # k_gemm<true> with a ragged K tile (100 = 3 * 32 + 4); N below one tile; one row tile + 1; k_dghat_part16 masking k < N inside its 64-feature step
    (17, 100, 36, 9, 63),     # k_dghat_part<1>, scalar loads (N % 8 = 4)
    (17, 40, 24, 9, 64),      # k_dghat_part<1>, 16-B loads (N % 8 = 0, N % 64 != 0)
    (32, 8, 64, 5, 9),        # J = 32: k_mix<8> both ways, k_dghat_part<1>; one 8-row group + 1
    (33, 8, 64, 7, 9),        # J = 33: k_gl5_mixm forward and <8, 1, true> transposed, k_dghat_part<2>; one 8-row group + 1
    (51, 12, 192, 43, 7),     # k_gl5_mixm with fewer than 8 rows, three column blocks
    (64, 100, 64, 1, 1),      # J = 64 (kMaxNodes), one row, one type
    (52, 16, 96, 4, 5),       # J > 32 with N % 64 != 0: launch_mix_mfma declines, k_mix<16>
    (5, 12, 20, 4, 513),      # three dW splits
    (5, 12, 20, 4, 2305),     # ten dW splits of kchunk 256, the last with one row
    (3, 4, 8, 3, 8200),       # the 32-split cap, kchunk 288: splits 29-31 empty (kbeg >= kend) and exactly zero; dghat, dbias and dW through k_sum_parts_wave
    (4, 192, 192, 2, 4100),   # dW with 17 splits and 73,728 elements: k_sum_parts at splits >= 16
]
DENSITY = {(4, 192, 192, 2, 4100): 1.0 / 16}  # see the module docstring
RANDOM_CASES = [c for c in GL_CASES if c[4] <= 513]
GUARD_CASES = [(21, 96, 3, 13, 37), (16, 100, 36, 10, 65), (33, 8, 64, 7, 9), (3, 4, 8, 3, 8200)]
SWEEP_ROWS = (1, 4, 5, 16, 17, 256, 257, 8192, 8193)

# variants of a case: one more type than the nodes use (the last, unused); all nodes of type 0; shared weights
# (n_types = 0); without bias
Variant = collections.namedtuple("Variant", "extra_type one_type shared bias", defaults=(False, False, False, True))
PLAIN = Variant()
VARIANT_CASES = [
    ((16, 100, 36, 10, 65), Variant(extra_type=True)),   # an unused type on the vector GEMMs
    ((21, 96, 3, 13, 37), Variant(extra_type=True)),     # ... on k_gemm<false>
    ((3, 4, 8, 3, 8200), Variant(extra_type=True)),      # ... with empty splits beside it
    ((17, 40, 24, 9, 64), Variant(one_type=True)),       # eight of nine types unused, one type takes all 17 nodes
    ((33, 8, 64, 7, 9), Variant(one_type=True)),
    ((16, 100, 36, 10, 65), Variant(shared=True)),
    ((16, 100, 36, 10, 65), Variant(shared=True, bias=False)),
    ((51, 12, 192, 43, 7), Variant(shared=True, bias=False)),
    ((5, 12, 20, 4, 513), Variant(bias=False)),
]
SUBSET_CASES = [(16, 100, 36, 10, 65), (33, 8, 64, 7, 9), (5, 12, 20, 4, 513)]
OFFSET_CASES = [(16, 100, 36, 10, 65), (17, 40, 24, 9, 64), (33, 8, 64, 7, 9)]


def case_id(case):
    return "-".join(str(v) for v in case)


def variant_id(v):
    return "+".join([f for f in ("extra_type", "one_type", "shared") if getattr(v, f)] + ([] if v.bias else ["nobias"]))


def ref_graph_linear(x, W, b, gh, types):
    """GraphLinear.forward of the reference with ghat given (per-type W, bias before the mixing)."""
    if types is not None:
        z = torch.einsum("noi,rni->rno", W[types], x)
        if b is not None:
            z = z + b[types]
    else:
        z = x @ W.t()
        if b is not None:
            z = z + b
    return gh.matmul(z), z


def _backward(x, W, b, gh, types, dy):
    """float64 autograd of ref_graph_linear: dict of y, z, dz and the four gradients (dbias None without b)."""
    leaves = [t.clone().requires_grad_(True) for t in (x, W, gh)] + ([b.clone().requires_grad_(True)] if b is not None else [])
    y, z = ref_graph_linear(leaves[0], leaves[1], leaves[3] if b is not None else None, leaves[2], types)
    z.retain_grad()
    y.backward(dy)
    return dict(y=y.detach(), z=z.detach(), dz=z.grad, dx=leaves[0].grad, dW=leaves[1].grad, dghat=leaves[2].grad,
                dbias=leaves[3].grad if b is not None else None)


def _node_types(J, nt, g):
    types = torch.randint(0, nt, (J,), generator=g)
    types[:nt] = torch.arange(nt)[: min(nt, J)]  # every type in use (nt <= J in the table)
    return types


Exact = collections.namedtuple("Exact", "x W b gh types dy n_types used ref sum_abs")


@functools.lru_cache(maxsize=None)
def exact_case(case, variant=PLAIN):
    """Inputs (float64, integer-valued) of a case, its float64 reference and `sum_abs`, the largest sum of |terms|
    of any element of y, z, dz, dx, dW, dbias and dghat.  `used`: the types some node has."""
    J, K, N, nt, rows = case
    g = torch.Generator().manual_seed(sum(v * 10 ** i for i, v in enumerate(case)) + 7919 * sum(int(f) << i for i, f in enumerate(variant)))
    hi = 2 if J < 33 else 1
    ints = lambda *shape: torch.randint(-hi, hi + 1, shape, generator=g).double()
    if variant.shared:
        nt = 0
    elif variant.extra_type:
        nt += 1
    x, dy = ints(rows, J, K), ints(rows, J, N)
    density = DENSITY.get(case, 1.0)
    if density < 1.0:
        x = x * (torch.rand(x.shape, generator=g) < density)
        dy = dy * (torch.rand(dy.shape, generator=g) < density)
    W = ints(nt, N, K) if nt else ints(N, K)
    b = (ints(nt, N) if nt else ints(N)) if variant.bias else None
    gh = torch.randint(-2, 3, (J, J), generator=g).double() / 2
    if J >= 2:  # negative entries, not symmetric, whatever the draw
        gh[0, 1], gh[1, 0] = -0.5, 1.0
    if not nt:
        types = None
    elif variant.one_type:
        types = torch.zeros(J, dtype=torch.int64)
    else:
        types = _node_types(J, nt - 1 if variant.extra_type else nt, g)
    used = sorted(set(types.tolist())) if nt else [0]
    ref = _backward(x, W, b, gh, types, dy)
    big = _backward(x.abs(), W.abs(), None if b is None else b.abs(), gh.abs(), types, dy.abs())
    sum_abs = max(float(v.max()) for v in big.values() if v is not None and v.numel())
    return Exact(x, W, b, gh, types, dy, nt, used, ref, sum_abs)


Random = collections.namedtuple("Random", "x W b G types dy n_types ref")


@functools.lru_cache(maxsize=None)
def random_case(case):
    """Uniform inputs as tests/test_training.py's kernel test draws them, a fully random G normalised in front
    (learn_influence), and float64 autograd through F.normalize: y and dx / dW / dG / dbias, and dghat, the gradient
    the kernel itself produces."""
    J, K, N, nt, rows = case
    g = torch.Generator().manual_seed(sum(v * 10 ** i for i, v in enumerate(case)) + 1)
    x = torch.rand(rows, J, K, generator=g, dtype=torch.float64) * 2 - 1
    W = (torch.rand((nt, N, K) if nt else (N, K), generator=g, dtype=torch.float64) * 2 - 1) / K ** 0.5
    b = torch.rand((nt, N) if nt else (N,), generator=g, dtype=torch.float64) - 0.5
    G = torch.rand(J, J, generator=g, dtype=torch.float64) * 2 - 1
    types = _node_types(J, nt, g) if nt else None
    dy = torch.rand(rows, J, N, generator=g, dtype=torch.float64) * 2 - 1
    leaves = [t.clone().requires_grad_(True) for t in (x, W, G, b)]
    gh = torch.nn.functional.normalize(leaves[2], p=1.0, dim=1)
    gh.retain_grad()
    y, _ = ref_graph_linear(leaves[0], leaves[1], leaves[3], gh, types)
    y.backward(dy)
    ref = dict(y=y.detach(), dx=leaves[0].grad, dW=leaves[1].grad, dG=leaves[2].grad, dbias=leaves[3].grad, dghat=gh.grad)
    return Random(x, W, b, G, types, dy, nt, ref)
