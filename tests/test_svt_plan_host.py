"""The SVT calls' resolved chain (lrs_diag_svt_plan, ops.svt_plan) against the table of its behaviour, on
every flag word at the band counts around each boundary; no GPU needed.

The table (Bp = B rounded up to even): Bp > 512, or Bp > 256 with MULTI_WG: unsupported.  Bp <= 256:
WIDE_TRI and WIDE_MW are ignored; JACOBI gives the Jacobi chain, otherwise MULTI_WG the many-workgroup
tridiagonal chain, otherwise the one-workgroup one.  Bp > 256: WIDE_TRI without JACOBI gives the wide
tridiagonal chain, which honours WIDE_MW; otherwise the wide Jacobi chain.  The warm-start products are formed
when WARM is set on a Jacobi chain; the state words are reset when the flag word without its ignored bits is
zero, or on a cold wide tridiagonal call."""
import ctypes

import pytest

from lrspnp import _lib, ops
from lrspnp._lib import LrsError

WARM, JACOBI, MULTI_WG, WIDE_TRI, WIDE_MW = 1, 2, 4, 8, 16
BANDS = (1, 199, 200, 201, 255, 256, 257, 258, 511, 512, 513)


def expected(B, flags):
    """The table above, transcribed; None where the calls refuse."""
    Bp = B + (B & 1)
    if Bp > 512 or (Bp > 256 and flags & MULTI_WG):
        return None
    if Bp <= 256:
        flags &= ~(WIDE_TRI | WIDE_MW)
        chain = "jacobi" if flags & JACOBI else "tri-multi-wg" if flags & MULTI_WG else "tri"
    else:
        chain = "wide-tri" if flags & WIDE_TRI and not flags & JACOBI else "wide-jacobi"
        if chain != "wide-tri":
            flags &= ~WIDE_MW
    warm = bool(flags & WARM)
    return dict(chain=chain, warm=warm, mw_reduction=chain == "wide-tri" and bool(flags & WIDE_MW),
                reset_state=flags == 0 or (chain == "wide-tri" and not warm),
                warm_products=warm and chain in ("jacobi", "wide-jacobi"))


def keywords(flags):
    return dict(warm=bool(flags & WARM), method="jacobi" if flags & JACOBI else "tri", multi_wg=bool(flags & MULTI_WG),
                wide_tri=bool(flags & WIDE_TRI), wide_mw=bool(flags & WIDE_MW))


@pytest.mark.parametrize("B", BANDS)
def test_plan_matches_the_table_on_every_flag_word(B):
    for flags in range(32):
        assert ops._svt_flags(**keywords(flags)) == flags
        want = expected(B, flags)
        if want is None:
            with pytest.raises(LrsError, match="LRS_E_UNSUPPORTED"):
                ops.svt_plan(B, **keywords(flags))
        else:
            assert ops.svt_plan(B, **keywords(flags)) == want, (B, flags)


def test_spare_words_are_zero_and_the_chain_ids_are_the_five():
    L = _lib.lib()
    seen = set()
    for B in BANDS[:-1]:
        for flags in range(32):
            out = (ctypes.c_int32 * 8)(*([-1] * 8))
            if L.lrs_diag_svt_plan(B, flags, out) == 0:
                assert list(out[5:]) == [0, 0, 0]
                seen.add(out[0])
    assert seen == {0, 1, 2, 3, 4}
    assert len(ops.SVT_CHAINS) == 5


@pytest.mark.parametrize("B,flags", [(513, 0), (300, MULTI_WG)])
def test_entry_points_refuse_before_any_device_work(B, flags):
    """LRS_E_UNSUPPORTED from the plan, with pointers that are never dereferenced (tests/test_svt_wide_abi.py)."""
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    big = 1 << 40
    out = (ctypes.c_int32 * 8)()
    assert L.lrs_diag_svt_plan(B, flags, out) == -2
    assert L.lrs_svt_gram_f32(fake, None, 1.0, 1000, B, flags, fake, big, None) == -2
    assert L.lrs_svt_finish_f32(fake, None, 1.0, 1000, B, 1.0, fake, None, flags, fake, big, None) == -2
    assert L.lrs_svt_f32(fake, None, 1.0, 1000, B, 1.0, fake, None, flags, fake, big, None) == -2
    if B > 512:   # the two diagnostic entries take no flag word: the band count alone refuses
        assert L.lrs_diag_svt_state(fake, 1000, B, fake) == -2
        assert L.lrs_diag_svt_apply(fake, None, 1.0, 1000, B, fake, fake, None) == -2
