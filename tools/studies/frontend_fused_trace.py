"""The offline front end with conv1 inside the row-block conv2 gather (masr_debug_set key 41 = 1: conv2_rows_kernel<1>) against
conv1_kernel + conv2_rows_kernel<0> (key 41 = 0), and the embed projection's K quarters on 64-row blocks (key 42 = 1:
conv2_rows_kernel<2>) against 128x128 tiles (key 42 = 0, gemm_f32_kernel<128, 128, 2, 4, 0, 2>), both keys alternating in one
process on the contract batch (B = 32 x 10 s) -- run it under `rocprofv3 --kernel-trace --stats` and compare the per-kernel
averages on the same box."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from masr_amd.engine import HipEngine
from masr_amd.utils import synthetic
e = HipEngine(synthetic.conformer_state_dict(0, 4233), vocab_size=4233)
pcm = torch.from_numpy(synthetic.synthetic_pcm(32, 160000, seed=1234)).cuda()
n = torch.full((32,), 160000, dtype=torch.int32, device='cuda')
for rep in range(6):
    for v in (1, 0):
        e.lib.masr_debug_set(e.h, 41, v)
        e.lib.masr_debug_set(e.h, 42, v)
        for _ in range(5):
            e.transcribe_batch(pcm, n)
        torch.cuda.synchronize()
