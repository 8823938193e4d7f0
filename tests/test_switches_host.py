"""The runtime switches (docs/SWITCHES.md): one table per side (csrc/switches.h, mmnas_amd/switches.py), one parser, one
setter path.  Host only.  Whatever depends on read-once state runs in a fresh child process; the children that need only the
native table load the shared library with plain ctypes (no torch import), so the module takes a few seconds."""
import json
import os
import re
import subprocess
import sys

import pytest

from tests.util import REPO

LIB = os.path.join(REPO, 'mmnas_amd', 'lib', 'libmmnas_hip.so')
DEFAULT, ENV, SET, UNREAD = 0, 1, 2, 4

# child code: the native table through the two enumeration calls, name -> [default, value, source]
INFO = r'''
def info():
    out = {}
    n, h, d, v, s = C.c_char_p(), C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
    for i in range(lib.mmnas_switch_count()):
        assert lib.mmnas_switch_info(i, C.byref(n), C.byref(h), C.byref(d), C.byref(v), C.byref(s)) == 0
        out[n.value.decode()] = [d.value, v.value, s.value]
    return out
'''
NATIVE = 'import ctypes as C, json, os, sys\nlib = C.CDLL(%r)\n' % LIB + INFO   # plain ctypes: no torch import


def _child(code, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith('MMNAS_')}
    e.update(env)
    p = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith(('{', '['))][-1])


def _native(**env):
    return _child(NATIVE + 'print(json.dumps(info()))\n', **env)


# ---------------------------------------------------------------------------------------- 1. completeness
CSRC = os.path.join(REPO, 'mmnas_amd', 'csrc')
# every getenv( left in csrc/: the switches implementation (util.hip) and the two string-valued rows, read through their row's name
GETENV_SITES = {('util.hip', 'name'), ('util.hip', 's.name'), ('util.hip', 'sw::prof_dump.name'), ('ops.hip', 'sw::side_flush.name')}
NOT_SWITCHES = ('MMNAS_DBG_',)   # compile-time -D names


def _sources(ext):
    for d, _, files in os.walk(os.path.join(REPO, 'mmnas_amd')):
        for f in files:
            if f.endswith(ext) and not os.path.basename(d).startswith('build'):
                yield os.path.join(d, f)


def test_every_variable_read_under_the_package_is_a_table_row():
    from mmnas_amd import switches as S
    rows = set(_native()) | set(S.TABLE)
    sites, named = set(), set()
    for path in list(_sources('.hip')) + list(_sources('.h')):
        src = re.sub(r'//[^\n]*|/\*.*?\*/', '', open(path).read(), flags=re.S)
        sites |= {(os.path.basename(path), a.strip()) for a in re.findall(r'\bgetenv\(([^()]*)\)', src)}
        named |= set(re.findall(r'"(MMNAS_[A-Z0-9_]+)"', src))
    assert sites == GETENV_SITES
    for path in _sources('.py'):
        src = open(path).read()
        named |= set(re.findall(r'''['"](MMNAS_[A-Z0-9_]+)['"]''', src))
        if os.path.basename(path) != 'switches.py':   # no module parses a variable of its own
            for line in src.splitlines():
                if 'os.environ' in line or 'getenv' in line:
                    assert not re.search(r'MMNAS_[A-Z0-9_]+', line.split('#')[0]), (path, line)
    named = {n for n in named if not n.startswith(NOT_SWITCHES)}
    assert len(named) >= 60 and named <= rows, sorted(named - rows)


# ---------------------------------------------------------------------------------------- 2. README
def test_readme_table_is_the_generated_one():
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    try:
        import switch_table
    finally:
        sys.path.pop(0)
    assert switch_table.readme_section(open(os.path.join(REPO, 'README.md')).read()) == switch_table.table()


# ---------------------------------------------------------------------------------------- 3. defaults
def test_defaults_with_nothing_set():
    t = _native()
    for name, (dflt, value, source) in t.items():
        assert value == dflt and source & 3 == DEFAULT, name
    want = {'CHAIN_OVERLAP': 0, 'REL_HOIST': 1, 'GUIDED_HOIST': 1, 'NODE_LNB': 1, 'SMALL_OPS': 1, 'SMALL_BWD': 1, 'SMALL_FFN': 0,
            'GEMM_LN': 0, 'GEMM_SPLIT': 6, 'GEMM_LEAN': 3, 'GEMM_PF': 2, 'MHA_FWD_B16_TWO': 320, 'REL_MULTI_WGS': 3,
            'REL_OVERLAP': 0, 'HEAD_OVERLAP': 0, 'HEAD_GLIMPSE1': 1, 'HEAD_PROJT': 1, 'REL_FWD_VALU': 0, 'SIDE_PRIO': 1,
            'GEMM_LN_MINM': 2048, 'GEMM_LN_MAXK': 256, 'MHA_NW': 4, 'MHA_PAIR': 1, 'MHA_BWD_FUSED': 1, 'MHA_FWD_B16': 1,
            'MHA_BWD_B16': 1, 'REL_MULTI_YIELD': 0, 'REL_BWD_VALU': 1, 'GEMM_TILE': 0, 'GEMM_GENERIC': 0, 'GEMM_SK': 1,
            'GEMM_MIN_UNITS': 4, 'GEMM_XCD': 1, 'GEMM_PAIR': 1, 'GEMM_SPLIT_P': 24, 'GEMM_SPLIT_MINWG': 256, 'GEMM_HYB_T': 16,
            'GEMM_LEAN_MAXB': 8 << 20, 'LSTM_FWD_P': 0, 'LSTM_BWD_P': 8}
    for k, v in want.items():
        assert t['MMNAS_' + k][1] == v, k
    py = _child('import json\nfrom mmnas_amd import switches as S\n'
                'print(json.dumps({k: [f.get(), f.default, f.info()["source"]] for k, f in S.TABLE.items() if f.policy != "doc"}))\n')
    for k, (value, dflt, source) in py.items():
        assert value == dflt and source == 'default', k
    want = {'CHAIN': True, 'MIXED_CHAIN': True, 'SIDE_STREAM': 0, 'AUTOGRAD_CHAIN': False, 'UNPAD': False, 'VGD_HEAD': False, 'LSTM': True,
            'CONV_IM2COL': None, 'HEAD_GLIMPSE1': True, 'GEMM_GENERIC': False, 'ZERO_TERMS': True, 'LAZY_REL': True, 'DP_ROWS': True,
            'DP_INLINE': True, 'DP_TAIL_MAIN': True, 'DP_EARLY_SCATTER': False}
    assert {k[6:]: v[0] for k, v in py.items()} == want


# ---------------------------------------------------------------------------------------- 4. parse table
BOOLS = ('CHAIN_OVERLAP', 'HEAD_OVERLAP', 'HEAD_GLIMPSE1', 'HEAD_PROJT', 'REL_HOIST', 'REL_OVERLAP', 'NODE_LNB', 'GUIDED_HOIST', 'SIDE_PRIO',
         'SMALL_OPS', 'SMALL_BWD', 'MHA_PAIR', 'MHA_BWD_FUSED', 'MHA_FWD_B16', 'MHA_BWD_B16', 'REL_BWD_VALU')
SETTERS = ('small_ops', 'small_bwd', 'small_ffn', 'chain_overlap', 'rel_hoist', 'guided_hoist', 'rel_overlap', 'gemm_ln')
# what the real read path (not the peek of mmnas_switch_info) gives: every setter reads its switch before it overrides it
READ_BY_SETTER = NATIVE + ('t = info()\n'
                           'print(json.dumps([t, {n: getattr(lib, "mmnas_set_" + n)(0) for n in %r}]))\n' % (SETTERS,))


@pytest.mark.parametrize('text', ['0', '1', ''])
def test_integer_and_boolean_switches_parse_0_1_and_empty(text):
    names = ['MMNAS_' + k for k in BOOLS + ('SMALL_FFN', 'GEMM_LN', 'REL_FWD_VALU', 'GEMM_XCD', 'GEMM_PAIR', 'GEMM_SK')]
    t, prev = _child(READ_BY_SETTER, **{n: text for n in names})
    for n in names:
        dflt, value, source = t[n]
        assert value == (dflt if text == '' else int(text)), n
        assert source & 3 == (DEFAULT if text == '' else ENV), n      # an empty variable is the default
    for s in SETTERS:
        assert prev[s] == t['MMNAS_' + s.upper()][1], s


def test_documented_integers_and_the_other_kinds():
    t, prev = _child(READ_BY_SETTER, MMNAS_SMALL_FFN='2', MMNAS_GEMM_TILE='128', MMNAS_GEMM_SPLIT='3', MMNAS_MHA_NW='2', MMNAS_GEMM_LN='2',
                     MMNAS_REL_FWD_VALU='2', MMNAS_GEMM_GENERIC='0', MMNAS_SIDE_FLUSH='op', MMNAS_GEMM_LN_MINM='896', MMNAS_REL_MULTI_YIELD='3')
    value = {k[6:]: v[1] for k, v in t.items()}
    assert value['SMALL_FFN'] == 2 and value['GEMM_TILE'] == 128 and value['GEMM_SPLIT'] == 3 and value['MHA_NW'] == 2
    assert value['GEMM_LN_MINM'] == 896 and value['REL_MULTI_YIELD'] == 3
    assert value['GEMM_LN'] == 0 and value['REL_FWD_VALU'] == 0           # on only for 1
    assert value['GEMM_GENERIC'] == 1                                     # on by presence: =0 is on
    assert value['SIDE_FLUSH'] == 1 and value['PROF_DUMP'] == 0           # string rows: set / not set
    assert prev['small_ffn'] == 2 and prev['gemm_ln'] == 0
    t, _ = _child(READ_BY_SETTER, MMNAS_GEMM_LN='1', MMNAS_REL_FWD_VALU='1')
    assert t['MMNAS_GEMM_LN'][1] == 1 and t['MMNAS_REL_FWD_VALU'][1] == 1 and t['MMNAS_GEMM_GENERIC'][1] == 0


def test_python_kinds(monkeypatch):
    """The every_call rows hold no state, so this process's own table serves."""
    from mmnas_amd import switches as S
    for text, want in ((None, 0), ('0', 0), ('1', 1), ('rel', 2)):
        monkeypatch.delenv('MMNAS_SIDE_STREAM', raising=False) if text is None else monkeypatch.setenv('MMNAS_SIDE_STREAM', text)
        assert S.SIDE_STREAM.get() == want
    for text, want in ((None, None), ('0', 0), ('1', 1)):       # conv_seq tells the three apart through this accessor
        monkeypatch.delenv('MMNAS_CONV_IM2COL', raising=False) if text is None else monkeypatch.setenv('MMNAS_CONV_IM2COL', text)
        assert S.CONV_IM2COL.get() == want and (S.CONV_IM2COL.get() is None) == (text is None)
    for f, unset in ((S.CHAIN, True), (S.LSTM, True), (S.ZERO_TERMS, True), (S.DP_ROWS, True), (S.AUTOGRAD_CHAIN, False), (S.DP_EARLY_SCATTER, False)):
        for text, want in ((None, unset), ('0', False), ('1', True)):
            monkeypatch.delenv(f.name, raising=False) if text is None else monkeypatch.setenv(f.name, text)
            assert f.get() is want, (f.name, text)
    monkeypatch.setenv('MMNAS_GEMM_GENERIC', '0')
    assert S.GEMM_GENERIC.get() is True


# ---------------------------------------------------------------------------------------- 5. setters
def test_native_setters_return_the_previous_value_and_are_reported():
    code = NATIVE + ('out = {}\n'
                     'for n in %r:\n'
                     '    f, key = getattr(lib, "mmnas_set_" + n), "MMNAS_" + n.upper()\n'
                     '    dflt = info()[key][0]\n'
                     '    first = f(1 - dflt); mid = info()[key]; second = f(first); end = info()[key]\n'
                     '    out[n] = [dflt, first, mid, second, end]\n'
                     'lib.mmnas_set_small_ffn(-1); lo = info()["MMNAS_SMALL_FFN"][1]\n'
                     'back = lib.mmnas_set_small_ffn(5); hi = info()["MMNAS_SMALL_FFN"][1]\n'
                     'out["clamp"] = [lo, back, hi, lib.mmnas_set_small_ffn(0)]\n'
                     'out["bad"] = [lib.mmnas_switch_info(-1, None, None, None, None, None), lib.mmnas_switch_info(lib.mmnas_switch_count(), None, None, None, None, None)]\n'
                     'print(json.dumps(out))\n' % (SETTERS,))
    out = _child(code)
    for n in SETTERS:
        dflt, first, mid, second, end = out[n]
        assert first == dflt                                    # the previous effective value: the default
        assert mid == [dflt, 1 - dflt, SET]                     # reported as set by call
        assert second == 1 - dflt and end == [dflt, dflt, SET]  # setting back restores
    assert out['clamp'] == [0, 0, 2, 2]
    assert out['bad'] == [-2, -2]


TORCH_CHILD = ('import ctypes as C, json, os\n'
               'from mmnas_amd import _lib as L, ops, switches as S\n'
               'lib = L.lib()\n'
               'out = {}\n')


def test_python_setters_and_runtime_config():
    code = TORCH_CHILD + ('before = ops.runtime_config()["switches"]\n'
                          'out["unpad"] = [ops.unpad_enabled(), ops.set_unpad(True), ops.unpad_enabled(), ops.set_unpad(False), ops.unpad_enabled()]\n'
                          'out["vgd"] = [ops.set_vgd_head(True), ops.vgd_head_enabled(), ops.set_vgd_head(False), ops.vgd_head_enabled()]\n'
                          'out["hoist"] = lib.mmnas_set_rel_hoist(0)\n'
                          'ops.set_unpad(True)\n'
                          'c = ops.runtime_config()\n'
                          'json.dumps(c)\n'
                          'out["keys"] = sorted(c)\n'
                          'out["before"] = [before["MMNAS_REL_HOIST"], before["MMNAS_UNPAD"]]\n'
                          'out["after"] = [c["switches"]["MMNAS_REL_HOIST"], c["switches"]["MMNAS_UNPAD"], c["switches"]["MMNAS_HEAD_GLIMPSE1"]]\n'
                          'out["n"] = [len(c["switches"]), lib.mmnas_switch_count(), len([f for f in S.TABLE.values() if f.policy != "doc"])]\n'
                          'print(json.dumps(out))\n')
    out = _child(code)
    assert out['unpad'] == [False, False, True, True, False]
    assert out['vgd'] == [False, True, True, False]
    assert out['hoist'] == 1
    assert {'env', 'switches', 'lib_path', 'abi_version', 'hip_force_dev_kernarg', 'hip_force_dev_kernarg_source'} <= set(out['keys'])
    assert out['before'] == [{'value': 1, 'default': 1, 'source': 'default', 'side': 'native'},
                             {'value': False, 'default': False, 'source': 'default', 'side': 'python'}]
    assert out['after'] == [{'value': 0, 'default': 1, 'source': 'set by call', 'side': 'native'},
                            {'value': True, 'default': False, 'source': 'set by call', 'side': 'python'},
                            {'value': 1, 'default': 1, 'source': 'default', 'side': 'both'}]
    assert out['n'][0] == out['n'][1] + out['n'][2] - 2       # two variables are read on both sides


# ---------------------------------------------------------------------------------------- 6. read timing, 7. both parsers
def test_read_timing():
    code = TORCH_CHILD + INFO + (
        # every_call: follows the environment after the library is loaded
        'a = [info()["MMNAS_HEAD_GLIMPSE1"], ops.chain_enabled(), ops.lstm_enabled()]\n'
        'os.environ.update(MMNAS_HEAD_GLIMPSE1="0", MMNAS_CHAIN="0", MMNAS_LSTM="0")\n'
        'b = [info()["MMNAS_HEAD_GLIMPSE1"], ops.chain_enabled(), ops.lstm_enabled()]\n'
        'os.environ.update(MMNAS_HEAD_GLIMPSE1="1", MMNAS_CHAIN="1", MMNAS_LSTM="1")\n'
        'out["every_call"] = [a, b, [info()["MMNAS_HEAD_GLIMPSE1"], ops.chain_enabled(), ops.lstm_enabled()]]\n'
        # once: MMNAS_GEMM_LN is read by the first product that asks whether the row-panel kernel applies -- here a descriptor
        # that does not qualify, refused on the host before anything is launched
        'os.environ["MMNAS_GEMM_LN"] = "1"\n'
        'peek = info()["MMNAS_GEMM_LN"]\n'
        'gd = L.GemmDesc()\n'
        'gd.layout, gd.ngroups, gd.nseg, gd.N, gd.K, gd.lda, gd.ldb, gd.ldc = L.GEMM_NN, 1, 1, 256, 256, 256, 256, 256\n'
        'one = C.c_void_p(16)\n'
        'rc = lib.mmnas_gemm_ln(C.byref(gd), one, one, one, 1e-6, None)\n'
        'read = info()["MMNAS_GEMM_LN"]\n'
        'os.environ["MMNAS_GEMM_LN"] = "0"\n'
        'os.environ["MMNAS_GEMM_LN_MINM"] = "7"\n'
        'out["once"] = [peek, rc, read, info()["MMNAS_GEMM_LN"], info()["MMNAS_GEMM_LN_MINM"], ops.unpad_enabled()]\n'
        'os.environ["MMNAS_UNPAD"] = "1"\n'
        'out["once"].append(ops.unpad_enabled())\n'
        # reload: the GEMM tuning follows the environment only at mmnas_gemm_reload_tuning()
        'lib.mmnas_gemm_reload_tuning()\n'
        'a = info()["MMNAS_GEMM_SPLIT"]\n'
        'os.environ["MMNAS_GEMM_SPLIT"] = "0"\n'
        'b = info()["MMNAS_GEMM_SPLIT"]\n'
        'lib.mmnas_gemm_reload_tuning()\n'
        'out["reload"] = [a, b, info()["MMNAS_GEMM_SPLIT"]]\n'
        'print(json.dumps(out))\n')
    out = _child(code)
    assert out['every_call'] == [[[1, 1, DEFAULT], True, True], [[1, 0, ENV], False, False], [[1, 1, ENV], True, True]]
    peek, rc, read, later, minm, unpad0, unpad1 = out['once']
    assert peek == [0, 1, ENV | UNREAD] and rc != 0
    assert read == [0, 1, ENV] and later == [0, 1, ENV]         # read once: the later change does not arrive
    assert minm == [2048, 2048, DEFAULT]                        # read together with MMNAS_GEMM_LN
    assert unpad0 is False and unpad1 is False
    assert out['reload'] == [[6, 6, DEFAULT], [6, 6, DEFAULT], [6, 0, ENV]]


def test_both_parsers_agree_where_both_sides_read_a_variable():
    code = NATIVE + ('from mmnas_amd import switches as S\n'
                     'out = []\n'
                     'for text in (None, "0", "1"):\n'
                     '    for k in ("MMNAS_HEAD_GLIMPSE1", "MMNAS_GEMM_GENERIC"):\n'
                     '        os.environ.pop(k, None)\n'
                     '        if text is not None: os.environ[k] = text\n'
                     '    lib.mmnas_gemm_reload_tuning()\n'
                     '    t = info()\n'
                     '    out.append([t["MMNAS_HEAD_GLIMPSE1"][1], int(S.HEAD_GLIMPSE1.get()), t["MMNAS_GEMM_GENERIC"][1], int(S.GEMM_GENERIC.get())])\n'
                     'print(json.dumps(out))\n')
    assert _child(code) == [[1, 1, 0, 0], [0, 0, 1, 1], [1, 1, 1, 1]]


# ---------------------------------------------------------------------------------------- 8. the fallback cases and the ledger
def _native_rows():
    """name -> [kind, default] of the native table ('[kind, policy] ...' opens every help text)."""
    code = NATIVE + ('out = {}\n'
                     'n, h, d, v, s = C.c_char_p(), C.c_char_p(), C.c_int(), C.c_int(), C.c_int()\n'
                     'for i in range(lib.mmnas_switch_count()):\n'
                     '    assert lib.mmnas_switch_info(i, C.byref(n), C.byref(h), C.byref(d), C.byref(v), C.byref(s)) == 0\n'
                     '    out[n.value.decode()] = [h.value.decode()[1:].split(",")[0], d.value]\n'
                     'print(json.dumps(out))\n')
    return _child(code)


def _parsed(kind, text):
    """What the native parser makes of a case's value (csrc/util.hip sw_parse), for the documented inputs the cases use."""
    if kind in ('presence', 'string'):
        return 1
    if kind == 'exact1':
        return int(text.startswith('1'))
    return int(text != '0') if kind == 'bool' else int(text)


def test_every_fallback_case_sets_native_rows_away_from_their_defaults():
    from tests import fallback_cases as F
    rows = _native_rows()
    assert len(F.CASES) >= 11
    for name, case in F.CASES.items():
        assert case['env'] and case['shapes'] and case['kind'] in F.RUNNERS, name
        assert F.REACHES.get(name), name      # every case says which kernels it is there for
        for k, text in case['env'].items():
            assert k in rows, (name, k)
            kind, dflt = rows[k]
            assert _parsed(kind, text) != dflt, (name, k, text, dflt)
        for shape in case['shapes']:
            assert F.bounds_of(name, shape)


# switches whose alternative side an existing test sets: variable -> (test file, how that file spells it when not by the
# variable's name or its mmnas_set_* setter: a keyword of test_kernels_gpu.py's gemm_tuning fixture)
COVERED_ELSEWHERE = {
    'MMNAS_CHAIN_OVERLAP': ('test_chain_gpu.py', None), 'MMNAS_HEAD_GLIMPSE1': ('test_chain_gpu.py', None),
    'MMNAS_REL_HOIST': ('test_chain_gpu.py', None), 'MMNAS_REL_OVERLAP': ('test_chain_gpu.py', None),
    'MMNAS_GUIDED_HOIST': ('test_chain_gpu.py', None), 'MMNAS_SMALL_OPS': ('test_small_gpu.py', None),
    'MMNAS_SMALL_BWD': ('test_small_gpu.py', None), 'MMNAS_SMALL_FFN': ('test_small_gpu.py', None),
    'MMNAS_GEMM_LN': ('test_gemm_ln_gpu.py', None),
    'MMNAS_HEAD_PROJT': ('test_fallback_paths_gpu.py', None), 'MMNAS_REL_FWD_VALU': ('test_fallback_paths_gpu.py', None),
    'MMNAS_GEMM_SPLIT': ('test_kernels_gpu.py', 'split=mode'), 'MMNAS_GEMM_TILE': ('test_kernels_gpu.py', 'tile=tile'),
    'MMNAS_GEMM_SK': ('test_kernels_gpu.py', 'sk=2'), 'MMNAS_GEMM_PAIR': ('test_kernels_gpu.py', 'pair=pair'),
    'MMNAS_GEMM_LEAN': ('test_kernels_gpu.py', None), 'MMNAS_GEMM_PF': ('test_kernels_gpu.py', 'pf=1'),
    'MMNAS_GEMM_XCD': ('test_kernels_gpu.py', 'xcd=0'), 'MMNAS_GEMM_GENERIC': ('test_kernels_gpu.py', 'generic=1'),
}
# switches nothing runs the other side of, with the reason (debug-build-only or pure tuning knobs only)
NOT_COVERED = {}
KERNEL_SELECTING_INTS = ('MMNAS_MHA_NW', 'MMNAS_REL_MULTI_YIELD', 'MMNAS_SMALL_FFN', 'MMNAS_GEMM_SPLIT', 'MMNAS_GEMM_TILE', 'MMNAS_GEMM_SK',
                         'MMNAS_GEMM_PF', 'MMNAS_GEMM_XCD', 'MMNAS_GEMM_PAIR', 'MMNAS_GEMM_LEAN')


def test_ledger_every_kernel_selecting_switch_has_a_test_of_its_other_side():
    """Every native switch of kind bool / exact1, and every int switch whose help names alternative kernels, is set by a case of
    tests/fallback_cases.py, by the existing test COVERED_ELSEWHERE names (checked: that file spells it), or is listed in
    NOT_COVERED with its reason.  A switch added without a test fails here."""
    from tests import fallback_cases as F
    rows = _native_rows()
    assert set(KERNEL_SELECTING_INTS) <= set(rows)
    need = {k for k, (kind, _) in rows.items() if kind in ('bool', 'exact1')} | set(KERNEL_SELECTING_INTS)
    by_case = {k for c in F.CASES.values() for k in c['env']}
    assert not (set(COVERED_ELSEWHERE) | set(NOT_COVERED)) - set(rows), 'a ledger entry that is no native switch'
    assert not set(NOT_COVERED) & (by_case | set(COVERED_ELSEWHERE))
    missing = need - by_case - set(COVERED_ELSEWHERE) - set(NOT_COVERED)
    assert not missing, sorted(missing)
    for k, (fname, spelled) in COVERED_ELSEWHERE.items():
        src = open(os.path.join(REPO, 'tests', fname)).read()
        setter = 'mmnas_set_' + k[len('MMNAS_'):].lower()
        if spelled is not None:
            assert k.startswith('MMNAS_GEMM_') and spelled.split('=')[0] == k[len('MMNAS_GEMM_'):].lower(), k
            assert 'def gemm_tuning' in src and re.search(r'gemm_tuning\([^)]*\b' + re.escape(spelled), src) or \
                re.search(r'dict\(' + re.escape(spelled) + r'\)', src), (k, fname)
        else:
            assert "'%s'" % k in src or setter in src, (k, fname)
    for k, why in NOT_COVERED.items():
        assert isinstance(why, str) and why.strip(), k


def test_fallback_runner_lists_its_cases_without_a_gpu():
    from tests import fallback_cases as F
    e = {k: v for k, v in os.environ.items() if not k.startswith('MMNAS_')}
    e['CUDA_VISIBLE_DEVICES'] = e['HIP_VISIBLE_DEVICES'] = ''
    p = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'fallback_cases.py'), '--list'], cwd=REPO, env=e,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    listed = [json.loads(l) for l in p.stdout.splitlines()]
    assert [r['case'] for r in listed] == list(F.CASES)
    for r in listed:
        c = F.CASES[r['case']]
        assert r['env'] == c['env'] and r['kind'] == c['kind'] and r['shapes'] == json.loads(json.dumps(c['shapes']))
    p = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'fallback_cases.py'), 'no_such_case'], cwd=REPO, env=e,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and 'usage' in p.stderr and not p.stdout


def test_fallback_references_against_torch():
    """The float64 references the runner judges the kernels by (tests/kernel_refs.py), on the CPU: the attention core against
    torch's scaled_dot_product_attention, and the relation bias's analytic gradients against a central difference."""
    import numpy as np
    import torch
    from tests.kernel_refs import mha_ref, rel_fused_ref
    rs = np.random.RandomState(5)
    B, H, Sq, Sk, dh = 2, 3, 5, 7, 8
    Q, K, V = (torch.from_numpy(rs.standard_normal((B, s, H * dh))) for s in (Sq, Sk, Sk))
    biasT = torch.from_numpy(rs.standard_normal((B, H, Sk, Sq)))
    mask = torch.zeros(B, Sk, dtype=torch.bool)
    mask[1, 4:] = True
    split = lambda t: t.reshape(B, -1, H, dh).permute(0, 2, 1, 3)
    am = biasT.permute(0, 1, 3, 2).masked_fill(mask.reshape(B, 1, 1, Sk), float('-inf'))
    want = torch.nn.functional.scaled_dot_product_attention(split(Q), split(K), split(V), attn_mask=am).permute(0, 2, 1, 3).reshape(B, Sq, H * dh)
    assert float((mha_ref(Q, K, V, mask, biasT, H, dh) - want).abs().max()) < 1e-12
    raw = rs.standard_normal((2, 3, 4, 4))
    Wy, by, Wr, br = rs.standard_normal((64, 4)) / 2, 0.1 * rs.standard_normal(64), rs.standard_normal((2, 64)) / 8, 0.1 * rs.standard_normal(2) + 1.0
    gb = rs.standard_normal((2, 2, 4, 3))
    bias, dWy, dby, dWr, dbr = rel_fused_ref(raw, Wy, by, Wr, br, gb)
    assert bias.shape == (2, 2, 4, 3)
    f = lambda b: float((rel_fused_ref(raw, Wy, by, Wr, b, gb)[0] * gb).sum())
    for h in range(2):
        e = np.zeros(2); e[h] = 1e-6
        assert abs((f(br + e) - f(br - e)) / 2e-6 - dbr[h]) < 1e-5 * max(1.0, abs(dbr[h]))
