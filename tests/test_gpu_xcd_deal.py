"""The premise gs_tuning "xcd_map" is built on: the dispatcher deals the workgroups of a launch round-robin over the XCDs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_workgroups_are_dealt_round_robin_over_the_xcds():
    """With "xcd_map" on, the render launches number their workgroups so that the four quadrant waves of a tile are 8 apart
    (common.h: render_block_map): they share an XCD, and with it an L2, only if the eight workgroups 8 r .. 8 r + 7 of a
    launch run on eight different XCDs.  On an MI355X in SPX mode the dispatcher deals workgroups round-robin, starting
    wherever the previous launch stopped: xcc[b] = (b + first) % 8.  A different deal would cost speed, never a wrong image
    -- but it is what the numbering is built on, so it is checked, over a few launches with different starting points."""
    from gsplat_mi355 import _lib
    firsts = set()
    for n in (4096, 13, 4096, 1027, 4096):
        x = _lib.xcc_probe(torch.device("cuda:0"), n).numpy()
        assert np.array_equal(x, (np.arange(n) + int(x[0])) % 8), x[:16]
        firsts.add(int(x[0]))
    assert set(_lib.xcc_probe(torch.device("cuda:0"), 64).numpy().tolist()) == set(range(8))
