"""The contract-size step (B = 32 x 10 s, transcribe_batch from PCM) of a Conformer with the conv2d6 and with the conv2d8
front-end (encoder_conf.input_layer), each after a conv2d run of the same weights' shapes -- run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel times: conv2d6's 5x5 stride-3 conv is conv2_rows_kernel<0, 5, 3>, conv2d8's
third conv a second conv2_rows_kernel<0, 3, 2> launch next to conv2d's fused <1, 3, 2>."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from masr_amd.engine import HipEngine
from masr_amd.utils import synthetic
pcm = torch.from_numpy(synthetic.synthetic_pcm(32, 160000, seed=1234)).cuda()
n = torch.full((32,), 160000, dtype=torch.int32, device='cuda')
for il in sys.argv[1:] or ('conv2d', 'conv2d6', 'conv2d8'):
    e = HipEngine(synthetic.conformer_state_dict(0, 4233, input_layer=il), encoder_conf={'input_layer': il}, vocab_size=4233)
    for _ in range(12):
        e.transcribe_batch(pcm, n)
    torch.cuda.synchronize()
    e.close()
