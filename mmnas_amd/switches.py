"""Runtime switches of the Python side: every MMNAS_* environment variable read under mmnas_amd/*.py is one row of TABLE
(the native library's rows: csrc/switches.h; the inventory of both: docs/SWITCHES.md; the README table is printed from
the two by tools/switch_table.py).

    kind      not0      on unless the value is exactly '0'                      -> bool
              is1       on only when the value is exactly '1' (the opt-in idiom) -> bool
              presence  on when the variable exists at all ('0' is on)           -> bool
              tri       '0' -> 0, '1' -> 1, anything else or unset -> None
              side      MMNAS_SIDE_STREAM: '1' -> 1, 'rel' -> 2, anything else -> 0
              string    read where it is used; the row documents it
    policy    every_call  read at every get()
              once        read at the first get(), then cached
              import      as once; the owning module reads it when it is imported
              doc         not read through this table (documentation row)

Flag.set installs an override that every later get() returns, whatever the policy, and returns the previous value.
"""
import contextlib
import os

_PARSE = {
    'not0': lambda v: v != '0',
    'is1': lambda v: v == '1',
    'presence': lambda v: v is not None,
    'tri': lambda v: int(v) if v in ('0', '1') else None,
    'side': lambda v: 2 if v == 'rel' else int(v == '1'),
    'string': lambda v: v,
}


class Flag:
    __slots__ = ('name', 'default', 'kind', 'policy', 'help', '_parse', '_state', '_value')

    def __init__(self, name, default, kind, policy, help):
        self.name, self.default, self.kind, self.policy, self.help = name, default, kind, policy, help
        self._parse = _PARSE[kind]
        self._state = None      # None: nothing cached; otherwise the source of _value
        self._value = None

    def get(self):
        if self._state is not None:
            return self._value
        v = self._parse(os.environ.get(self.name))
        if self.policy != 'every_call':
            self._value, self._state = v, 'environment' if self.name in os.environ else 'default'
        return v

    def set(self, v):
        prev = self.get()
        self._value, self._state = v, 'set by call'
        return prev

    def info(self):
        """{value, default, source} without caching anything (a switch not read yet reports what a read now would give)."""
        if self._state is not None:
            return {'value': self._value, 'default': self.default, 'source': self._state}
        return {'value': self._parse(os.environ.get(self.name)), 'default': self.default,
                'source': 'environment' if self.name in os.environ else 'default'}


def _flag(*a):
    f = Flag(*a)
    TABLE[f.name] = f
    return f


TABLE = {}
CHAIN = _flag('MMNAS_CHAIN', True, 'not0', 'every_call', '0: one autograd node per operator instead of the backbone chain')
MIXED_CHAIN = _flag('MMNAS_MIXED_CHAIN', True, 'not0', 'every_call', '0: the architecture step on the per-candidate path (one node per candidate + MixedSumFn)')
SIDE_STREAM = _flag('MMNAS_SIDE_STREAM', 0, 'side', 'every_call', "1: the chain's weight-gradient work on a second stream; rel: only the relation-bias backward; measured slower (DESIGN.md)")
AUTOGRAD_CHAIN = _flag('MMNAS_AUTOGRAD_CHAIN', False, 'is1', 'every_call', '1: the chain as one autograd node whose inputs are the parameters (stock DDP); measured neutral')
UNPAD = _flag('MMNAS_UNPAD', False, 'is1', 'once', '1: the decoder stream on the valid region rows only (ops.set_unpad): same logits and gradients, supernet step 4.73 -> 3.78 ms (DESIGN.md)')
VGD_HEAD = _flag('MMNAS_VGD_HEAD', False, 'is1', 'once', '1: the grounding head as one native call per direction (ops.set_vgd_head); measurement: README, the grounding head section')
LSTM = _flag('MMNAS_LSTM', True, 'not0', 'every_call', '0: nn.LSTM (MIOpen, ~110 launches per step) instead of the persistent-kernel LSTM')
CONV_IM2COL = _flag('MMNAS_CONV_IM2COL', None, 'tri', 'every_call', 'dense Conv1d: 1 always through the window buffer, 0 direct whenever the shape allows, unset: direct unless the padded grid costs > 25 % more rows')
HEAD_GLIMPSE1 = _flag('MMNAS_HEAD_GLIMPSE1', True, 'not0', 'every_call', '0: one-unit linear layers as GEMM launches (A/B, tests); the native head reads it too')
GEMM_GENERIC = _flag('MMNAS_GEMM_GENERIC', False, 'presence', 'every_call', 'set (to anything): dense Conv1d through the window buffer, as the guarded-load GEMM path needs; gemm.hip reads it too')
ZERO_TERMS = _flag('MMNAS_ZERO_TERMS', True, 'not0', 'every_call', "0: plain parameters instead of the zero-term bookkeeping of the reference's literal lines (zeroterm.py)")
LAZY_REL = _flag('MMNAS_LAZY_REL', True, 'not0', 'import', '0: materialise the relation embeddings as the reference does (read when model/nets.py is imported)')
DP_ROWS = _flag('MMNAS_DP_ROWS', True, 'not0', 'every_call', '0: the embedding gradient exchanged dense instead of by rows (A/B)')
DP_INLINE = _flag('MMNAS_DP_INLINE', True, 'not0', 'every_call', '0: async_op=True + work.wait() instead of collectives issued inline on the communication stream')
DP_TAIL_MAIN = _flag('MMNAS_DP_TAIL_MAIN', True, 'not0', 'import', '0: the end of a data-parallel step on the communication stream, one scatter per bucket (1: -0.7 % on search_vqa_dp1; read when dp.py is imported)')
DP_EARLY_SCATTER = _flag('MMNAS_DP_EARLY_SCATTER', False, 'is1', 'every_call', "1: scatter a bucket's averaged gradients back as soon as its all-reduce is done")
LIB_PATH = _flag('MMNAS_LIB_PATH', None, 'string', 'doc', 'path of the shared library to load instead of mmnas_amd/lib/libmmnas_hip.so (tuning builds; read when _lib.py is imported)')
_flag('MMNAS_REFERENCE_ROOT', None, 'string', 'doc', "a checkout of the reference whose mmnas/ package is merged behind this repository's (mmnas/__init__.py)")
_flag('MMNAS_PROF_DUMP', None, 'string', 'doc', 'file the native profiler appends one row per bracketed launch to (csrc/util.hip)')
_flag('MMNAS_LN_ROWS_STATS', None, 'string', 'doc', 'file tests/test_ln_rows_gpu.py writes the worst LayerNorm error per (kernel, row class, output) to (tests/ln_rows.py)')
_flag('MMNAS_PACKED_HEADS_STATS', None, 'string', 'doc', 'file tests/test_ragged_heads_gpu.py writes the worst ragged-against-padded error per case to (heads of 16 / 32 / 128 / 256 on the ragged streams)')


@contextlib.contextmanager
def gemm_schedule(rows):
    """The native library's GEMM scheduling rows (policy `reload` in csrc/switches.h) at the given values while the block runs --
    gemm_schedule({'MMNAS_GEMM_SK': 0}): whole output tiles, no stream-K -- and as they were afterwards.  The library reads these
    rows from the environment, so that is where the values go; mmnas_gemm_reload_tuning makes it read them again."""
    from . import _lib as L
    known = native()
    for name in rows:
        if name not in known:
            raise ValueError('gemm_schedule: %s is not a row of the native switch table' % name)
    saved = {}
    try:
        for name, v in rows.items():
            saved[name] = os.environ.get(name)
            os.environ[name] = str(int(v))
        L.lib().mmnas_gemm_reload_tuning()
        yield
    finally:
        for name, v in saved.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
        L.lib().mmnas_gemm_reload_tuning()


def native():
    """The native library's table through mmnas_switch_info: name -> {value, default, source, help, read}.  Caches nothing."""
    import ctypes as C
    from . import _lib as L
    lib = L.lib()
    out = {}
    name, text, dflt, value, source = C.c_char_p(), C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
    for i in range(lib.mmnas_switch_count()):
        L.check(lib.mmnas_switch_info(i, C.byref(name), C.byref(text), C.byref(dflt), C.byref(value), C.byref(source)))
        out[name.value.decode()] = {'value': value.value, 'default': dflt.value, 'source': ('default', 'environment', 'set by call')[source.value & 3],
                                    'read': not source.value & 4, 'help': text.value.decode()}
    return out


def report():
    """Both tables for ops.runtime_config(): name -> {value, default, source, side}.  A variable both sides read
    (MMNAS_HEAD_GLIMPSE1, MMNAS_GEMM_GENERIC) is reported from the native table, side 'both'."""
    out = {}
    for k, r in native().items():
        out[k] = {'value': r['value'], 'default': r['default'], 'source': r['source'], 'side': 'native'}
    for k, f in TABLE.items():
        if k in out:
            out[k]['side'] = 'both'
        elif f.policy != 'doc':
            out[k] = dict(f.info(), side='python')
    return out
