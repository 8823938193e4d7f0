"""The attention cores' limits without a GPU: no key limit any more, the remaining limits answered on the host before any
launch, and the switch MMNAS_MHA_STREAM_MINK in the native table.  Drives the loaded library with descriptors that never reach
a kernel (null or dummy pointers)."""
import ctypes as C
import json
import os
import subprocess
import sys

from tests.util import REPO

E_SHAPE, E_ARG = -1, -2


def _desc(L, B, H, Sq, Sk, dh):
    d = L.MhaDesc()
    d.B, d.H, d.Sq, d.Sk, d.dh = B, H, Sq, Sk, dh
    d.ldq = d.ldk = d.ldv = d.ldo = H * dh
    return d


def _dummy(L, d):
    """16-byte-aligned addresses that are never dereferenced: the checks under test answer before any launch."""
    for k in ('Q', 'K', 'V', 'O', 'lse'):
        setattr(d, k, 4096)
    return d


def test_257_keys_pass_the_shape_checks():
    from mmnas_amd import _lib as L
    lib = L.lib()
    d = _desc(L, 2, 2, 5, 257, 64)
    for call in (lib.mmnas_mha_core_fwd, lib.mmnas_mha_core_bwd):
        assert call(C.byref(d), None) == E_ARG          # the null-pointer check, which follows the shape checks
        msg = lib.mmnas_last_error()
        assert b'256 keys' not in msg and b'null' in msg, msg
    for Sk in (1024, 4096):
        assert lib.mmnas_mha_core_fwd(C.byref(_desc(L, 2, 2, 5, Sk, 16)), None) == E_ARG


def test_the_remaining_limits_answer_before_any_launch():
    from mmnas_amd import _lib as L
    lib = L.lib()
    d = _dummy(L, _desc(L, 64, 8, 4096, 2048, 64))          # B H Sq Sk = 2^32: the dropout / bias index is 32-bit
    assert lib.mmnas_mha_core_fwd(C.byref(d), None) == E_SHAPE
    assert b'score tensor too large' in lib.mmnas_last_error()
    d = _dummy(L, _desc(L, 2, 2, 100, 300, 64))              # packed rows: d_h = 64 and at most 128 queries / keys
    d.q_off = 4096
    assert lib.mmnas_mha_core_fwd(C.byref(d), None) == E_SHAPE
    assert b'packed rows' in lib.mmnas_last_error()
    assert lib.mmnas_mha_core_fwd(C.byref(_desc(L, 2, 2, 5, 300, 48)), None) == E_SHAPE      # head dims as before
    assert b'head dim' in lib.mmnas_last_error()
    d = _dummy(L, _desc(L, 2, 2, 5, 300, 64))
    d.ldk = 2 * 64 + 2
    assert lib.mmnas_mha_core_fwd(C.byref(d), None) == E_SHAPE                                  # strides as before


CHILD = r'''
import ctypes as C, json
lib = C.CDLL(%r)
n, h, d, v, s = C.c_char_p(), C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
out = {}
for i in range(lib.mmnas_switch_count()):
    assert lib.mmnas_switch_info(i, C.byref(n), C.byref(h), C.byref(d), C.byref(v), C.byref(s)) == 0
    if n.value == b'MMNAS_MHA_STREAM_MINK':
        out = {'default': d.value, 'value': v.value, 'source': s.value, 'help': h.value.decode()}
print(json.dumps(out))
'''


def _switch(**env):
    lib = os.path.join(REPO, 'mmnas_amd', 'lib', 'libmmnas_hip.so')
    e = {k: v for k, v in os.environ.items() if not k.startswith('MMNAS_')}
    e.update(env)
    p = subprocess.run([sys.executable, '-c', CHILD % lib], cwd=REPO, env=e, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.splitlines()[-1])


def test_switch_row_default_and_environment():
    row = _switch()
    assert row and row['default'] == 257 and row['value'] == 257 and row['source'] & 3 == 0
    assert row['help'].startswith('[int, every_call]')
    row = _switch(MMNAS_MHA_STREAM_MINK='64')
    assert row['default'] == 257 and row['value'] == 64 and row['source'] & 3 == 1
