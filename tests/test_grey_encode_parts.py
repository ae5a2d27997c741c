"""Encode grey in sub-batches: with NHW_PARTS=2 a batch of 512 pictures or more runs its stages behind the front as two
sub-batches, each of which starts at its own picture of the input -- 262144 bytes a picture here, not 786432.  The batch repeats five pictures, so
a stride of three pictures lands on another picture wherever i % 5 != 0.  n = 517 is the smallest odd split above the threshold."""
import os

import pytest

from tests.grey_encode_cases import SEEDS, oracle_file, synth_grey


@pytest.mark.gpu
@pytest.mark.parametrize("q", [18, 23])
def test_grey_sub_batches_on_streams_match_oracle(oracle, q):
    import numpy as np
    import torch
    import nhwcodec_amd
    n = 517
    os.environ["NHW_PARTS"] = "2"
    try:
        e = nhwcodec_amd.Encoder(0, max_batch=n)
    finally:
        del os.environ["NHW_PARTS"]
    five = torch.from_numpy(np.stack([synth_grey(s) for s in SEEDS])).cuda()
    grey = five[torch.arange(n, device="cuda") % 5].contiguous()
    o, sizes, status = e.encode_grey_device(grey, q)
    torch.cuda.synchronize()
    assert e.timing().parts == 2
    assert int((status != 0).sum()) == 0
    sz = sizes.cpu().numpy()
    for i in (0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1):
        assert o[i, : sz[i]].cpu().numpy().tobytes() == oracle_file(oracle, synth_grey(SEEDS[i % 5]), q), f"picture {i}"
    e.close()
