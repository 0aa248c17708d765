"""CPU: functional.dx3_tile_lists -- the tile lists of a gradient that is zero outside row ``b*S + r0`` of every sample -- against a
brute-force scan of the rows, and the claim registry that says which tensor carries such a pattern."""
import pytest
import torch

import xpretrain_amd.functional as XF


def _scan(B, S, r0):
    """the 64-row tiles that hold a non-zero row, found by looking at every row"""
    hot = torch.zeros(B * S, dtype=torch.bool)
    hot[torch.arange(B) * S + r0] = True
    pad = (-hot.numel()) % 64
    return set(torch.nonzero(torch.cat([hot, hot.new_zeros(pad)]).view(-1, 64).any(1)).flatten().tolist())


CASES = [
    (8, 2356, 0, [(3, 6336), (3, 6336), (12, 1600)]),      # the step's last video layer: dW2, dW1, dWo
    (2, 4120, 0, [(3, 2752), (3, 2752), (12, 704)]),        # a slab with no active tile at split 3; S no multiple of 64
    (4, 100, 0, [(1, 448), (2, 256)]),                      # two samples share a 256-row tile; the last tile is partial (400 rows)
    (3, 333, 332, [(2, 512), (4, 256)]),                    # r0 = the sample's last row; 999 rows
    (1, 130, 129, [(1, 192)]),                              # the only active tile is the partial K tail
]


@pytest.mark.parametrize("B,S,r0,slabs", CASES)
def test_lists_against_a_row_scan(B, S, r0, slabs):
    rows = B * S
    active = _scan(B, S, r0)
    m_tiles, lists = XF.dx3_tile_lists(B, S, r0, slabs)
    assert len(lists) == len(slabs)
    union = set()
    for (split, kps), (tiles, begin) in zip(slabs, lists):
        assert len(begin) == split + 1 and begin[0] == 0 and begin[-1] == len(tiles)
        for z in range(split):
            mine = tiles[begin[z]:begin[z + 1]]
            k0, k1 = z * kps // 64, (min((z + 1) * kps, rows) + 63) // 64
            assert len(mine) >= 2, "the pipeline depth"
            assert mine == sorted(set(mine)), "ascending, no tile twice"
            assert all(k0 <= kt < k1 for kt in mine), "a slab walks its own k range"
            assert {kt for kt in active if k0 <= kt < k1} <= set(mine), "an active tile is missing"
            padding = set(mine) - active
            assert len(padding) == max(0, 2 - len(set(mine) & active)), "padding only up to the pipeline depth"
        assert active <= set(tiles)
        union |= set(tiles)
    assert m_tiles == sorted({kt // 4 for kt in union})
    assert all(0 <= t < (rows + 255) // 256 for t in m_tiles)


def test_a_slab_shorter_than_the_pipeline_is_refused():
    with pytest.raises(ValueError):
        XF.dx3_tile_lists(1, 64, 0, [(1, 64)])


def test_claims_follow_the_tensor_object_and_its_version():
    t = torch.zeros(12, 4)
    assert XF.row_support_of(t) is None
    XF.claim_row_support(t, 3, 4, 0)
    assert XF.row_support_of(t) == (3, 4, 0)
    assert XF.row_support_of(t.clone()) is None and XF.row_support_of(t + 0) is None      # a sum of gradients is another tensor
    assert XF.row_support_of(t.view(12, 4)) is None                                       # ... and so is a view
    t[5].add_(1.0)                                                                        # an in-place write bumps the version
    assert XF.row_support_of(t) is None
    u = torch.zeros(12, 4)
    XF.claim_row_support(u, 3, 4, 0)
    key = id(u)
    del u
    assert key not in XF._ROW_CLAIMS, "a dead tensor leaves no claim behind for whoever reuses its id"
