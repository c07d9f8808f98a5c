"""CPU: TXE_WALK_NO_REFORM, the `phases` bit of txe_gat_collapse_bwd_fused that include/txe.h keeps in an enum of its own, has the same
value in _lib.py and collides with no other bit that call takes."""
from test_cabi import _header_constants


def test_the_reform_bit_matches_the_header_and_is_a_free_bit():
    from taxoexpan_amd import _lib
    hdr = _header_constants()
    bit = hdr["TXE_WALK_NO_REFORM"]
    assert _lib.WALK_NO_REFORM == bit and bit > 0 and bit & (bit - 1) == 0
    others = [v for k, v in hdr.items() if k.startswith(("TXE_FUSED_", "TXE_PH_"))]
    assert len(others) >= 10 and all(v & bit == 0 for v in others)
