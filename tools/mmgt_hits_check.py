"""tools/bench_mmgt.py found another hit count for torch's chunked no-matmul cdist than for sd_cdist at the AMASS
shape (12,727 x 63, the bench's synthetic clusters).  This decides which side moves: every one of the N^2 pairs is
also evaluated in float64 from differences, and `d < thr` of sd_cdist and of torch.cdist, each as one call and in
row chunks of 2048, is compared with it entry by entry (output: profiles/mmgt/hits_check.txt).

Usage: python tools/mmgt_hits_check.py"""
import sys

import torch

sys.path.insert(0, ".")
from skeletondiffusion_amd import multimodal_gt  # noqa: E402

cuda = torch.device("cuda:0")
N, D0, THR, CHUNK, members = 12727, 63, 0.5, 2048, 48
g = torch.Generator().manual_seed(N)
centres = torch.randn((N + members - 1) // members, D0, generator=g) * 0.3
obs = (centres[torch.arange(N) // members] + torch.randn(N, D0, generator=g) * (0.05 * (48 / D0) ** 0.5)).to(cuda)
NO_MM = "donot_use_mm_for_euclid_dist"
full_h = multimodal_gt.cdist(obs, obs)
full_t = torch.cdist(obs, obs, p=2, compute_mode=NO_MM)
x64 = obs.double()
tot = {"hip_full": 0, "torch_full": 0, "torch_chunk": 0, "hip_chunk": 0, "f64": 0}
wrong = {"hip_full": 0, "torch_full": 0, "torch_chunk": 0, "hip_chunk": 0}
for r0 in range(0, N, CHUNK):
    r1 = min(N, r0 + CHUNK)
    ref = torch.cat([((x64[a:min(a + 128, r1), None] - x64[None]) ** 2).sum(-1).sqrt() for a in range(r0, r1, 128)]) < THR
    sides = {"hip_full": full_h[r0:r1] < THR, "torch_full": full_t[r0:r1] < THR,
             "torch_chunk": torch.cdist(obs[r0:r1], obs, p=2, compute_mode=NO_MM) < THR,
             "hip_chunk": multimodal_gt.cdist(obs[r0:r1], obs) < THR}
    tot["f64"] += int(ref.sum())
    for k, v in sides.items():
        tot[k] += int(v.sum())
        wrong[k] += int((v != ref).sum())
    tc = torch.cdist(obs[r0:r1], obs, p=2, compute_mode=NO_MM)
    print(r0, "max |torch chunk - torch full|", float((tc - full_t[r0:r1]).abs().max()), "max |hip chunk - hip full|",
          float((multimodal_gt.cdist(obs[r0:r1], obs) - full_h[r0:r1]).abs().max()), flush=True)
print("hits", tot)
print("entries that disagree with float64", wrong)
