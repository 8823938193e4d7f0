"""The chain planner's checks of a ragged language stream (x_off), on the host: mmnas_chain_plan runs chain_check before it lays
anything out, so no device is needed (tests/host_plan_driver.py: fake, never dereferenced pointers).  Packed keys no longer ask for
heads of 64; an encoder operator with a relation bias is refused as before."""
import ctypes as C

from tests.host_plan_driver import FAKE, att_record, chain, mlp_record

MMNAS_OK, MMNAS_E_ARG = 0, -2


def _chain_x_ragged(L, guided_dh, enc_rel):
    d = 256
    enc = att_record(L, 0, True, enc_rel, d, node=0)
    ff = mlp_record(L, 0, d, node=1)
    gd = att_record(L, 1, False, False, d, node=2)
    gd.att.dh, gd.att.H = guided_dh, d // guided_dh
    ch, keep = chain(L, [enc, ff, gd], B=5, Sx=20, Sy=23, d=d)
    ch.x_off, ch.Nx = FAKE, 50
    return ch, keep


def test_packed_keys_plan_at_heads_of_32():
    from mmnas_amd import _lib as L
    lib = L.lib()
    sz = C.c_size_t()
    ch, keep = _chain_x_ragged(L, 32, False)
    rc = lib.mmnas_chain_plan(C.byref(ch), C.byref(sz))
    assert rc == MMNAS_OK, lib.mmnas_last_error().decode()
    assert sz.value > 0
    for dh in (16, 128, 256):
        ch, keep = _chain_x_ragged(L, dh, False)
        assert lib.mmnas_chain_plan(C.byref(ch), C.byref(sz)) == MMNAS_OK, (dh, lib.mmnas_last_error().decode())


def test_encoder_relation_bias_is_still_refused():
    from mmnas_amd import _lib as L
    lib = L.lib()
    sz = C.c_size_t()
    ch, keep = _chain_x_ragged(L, 32, True)
    assert lib.mmnas_chain_plan(C.byref(ch), C.byref(sz)) == MMNAS_E_ARG
    assert 'relation bias' in lib.mmnas_last_error().decode()
