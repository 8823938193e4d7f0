"""The launch schedule of the backbone chains (mmnas_chain_fwd / _bwd, plain and mixed: ops.hip) against a recorded one.

The equality tests compare numbers; none of them would notice a launch that moved, doubled or went missing as long as the
numbers still agree.  Here each configuration runs ONE forward + backward under the native profiler (mmnas_prof_enable(1)) and
collects with MMNAS_PROF_DUMP pointing at a temporary file (the variable is read at every collect): one row per bracketed
launch, in issue order.  Of each row the test keeps (kind, tag, flops, bytes) -- the milliseconds are dropped -- and the
sequence must equal tests/golden/chain_schedule.json EXACTLY.

What is recorded: only launches inside a ProfScope appear -- 35 scopes over the library's 146 launch sites, covering the GEMM,
attention, relation, row, LSTM, small and head classes; stem, head and loss launches of the step are in the sequence next to the
chain's.  Copies and memsets do not appear, nor do event records and waits: a stream assignment shows only through the order in
which the host issued the launches.

Where the golden comes from: from the PARENT commit's library, never from the code under test.  Build the parent's csrc into a
library of its own, point MMNAS_LIB_PATH at it and run this file with MMNAS_REGEN_SCHEDULE=1: every configuration that ran
rewrites its entry (and the test passes without comparing).  A pull request that changes the schedule on purpose regenerates
the file from its own library instead and shows the diff of the JSON, which then is the review of the new schedule.  The one
entry marked "recorded_from": "this change" (arch_full_small_bwd0) had no parent to record from: a mixed chain whose sampled
candidate took the one-launch forward but not the one-launch backward returned an error before the change that added it.

Configurations: the sizes of the existing equality tests (weight step and Net_Full B=3, Sx=6, Sy=9; architecture step B=3,
Sx=5, Sy=7) at HSIZE 256, the smallest width that reaches the short-sequence kernels and the node's fused LayerNorm backward;
dropout 0.1, fixed seeds.  Switches go through their setters and are restored."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'chain_schedule.json')
ONLY_THIS_CHANGE = ('arch_full_small_bwd0',)

# name -> (step, native setters {name: value}, MMNAS_SIDE_STREAM, ragged decoder stream)
#   step: 'weight' = supernet weight step, plan seed 1; 'net_full' = Net_Full mmnas_vqa; 'arch_full' / 'arch_two' = the
#   architecture step through the mixed chain, plan seed 6
CONFIGS = {
    'weight': ('weight', {}, '0', False),
    'weight_side_1': ('weight', {}, '1', False),
    'weight_side_rel': ('weight', {}, 'rel', False),
    'net_full': ('net_full', {}, '0', False),
    'arch_full': ('arch_full', {}, '0', False),
    'arch_two': ('arch_two', {}, '0', False),
    'weight_rel_overlap': ('weight', {'rel_overlap': 1}, '0', False),
    'arch_full_rel_overlap': ('arch_full', {'rel_overlap': 1}, '0', False),
    'weight_chain_overlap': ('weight', {'chain_overlap': 1}, '0', False),
    'weight_rel_hoist0': ('weight', {'rel_hoist': 0}, '0', False),
    'arch_full_rel_hoist0': ('arch_full', {'rel_hoist': 0}, '0', False),
    'weight_guided_hoist0': ('weight', {'guided_hoist': 0}, '0', False),
    'arch_full_guided_hoist0': ('arch_full', {'guided_hoist': 0}, '0', False),
    'weight_ragged': ('weight', {}, '0', True),
    'arch_full_small_bwd0': ('arch_full', {'small_bwd': 0}, '0', False),
}


def _net(cls, c):
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = cls(c['cfg'], init)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in c['P'].items()})
    return net.to(DEV).train()


def _one_step(step, ragged):
    """Builds the net, then runs one forward + backward with the profiler on and collects (which writes the dump)."""
    import mmnas_amd._lib as L
    from mmnas.model.mixed import MixedOp
    from mmnas_amd import dp, ops
    from mmnas_amd.harness import SearchLoop
    lib = L.lib()
    arch = step.startswith('arch_')
    if step == 'net_full':
        c = cases.net_case('vqa', 'mmnas_vqa', 31337, HSIZE=256, B=3, Sx=6, Sy=9)
        cls = importlib.import_module('mmnas.model.full_vqa').Net_Full
    else:
        c = cases.net_case('vqa', None, 4242 if arch else 31337, search=True, HSIZE=256, B=3, Sx=5 if arch else 6, Sy=7 if arch else 9)
        cls = importlib.import_module('mmnas.model.hygr_vqa').Net_Search
    c['cfg'].DROPOUT_R = 0.1
    net = _net(cls, c)
    inp = tuple(torch.from_numpy(a).to(DEV) for a in c['inputs'])
    tgt = torch.from_numpy(c['target']).to(DEV)
    if ragged:      # lengths that differ per sample, every sample with a padded tail or full
        lens = [int((a != 0).any(-1).sum()) for a in c['inputs'][0]]
        assert len(set(lens)) > 1 and min(lens) > 0, lens
    seen = []
    orig_apply = ops.BackboneFn.apply
    ops.BackboneFn.apply = lambda *a: (seen.append(a[10] is not None), orig_apply(*a))[1]
    ops.manual_seed(99)
    sinks = None
    arr = (L.ProfStat * len(L.K_NAMES))()
    L.check(lib.mmnas_prof_enable(1))
    try:
        if arch:
            pl = cases.search_plan(np.random.RandomState(6), step[len('arch_'):])
            plan = pl['enc'] + pl['dec']
            if step == 'arch_full':     # (what arch_full_small_bwd0 is there for: a sampled SelfAtt on the language stream)
                assert any(act == [0] for act, _ in pl['enc']), pl['enc']
            loop = SearchLoop(net, arch_mode=step[len('arch_'):])
            sinks = loop.reducer.fg
            loop.arch_step(inp, tgt, plan=plan)
        else:
            if step == 'weight':
                pl = cases.search_plan(np.random.RandomState(1), None)
                MixedOp.MODE = None
                net.set_sampled(pl['enc'] + pl['dec'])
                red = dp.SupernetReducer(net)
                red.begin_weight_step()
            else:
                red = dp.GradReducer(list(net.parameters()))
                red.begin_step()
            sinks = red.fg
            loss = torch.nn.functional.binary_cross_entropy_with_logits(net(inp), tgt, reduction='sum')
            loss.backward()
            red.finish_weight_step() if step == 'weight' else red.finish()
        torch.cuda.synchronize()
        L.check(lib.mmnas_prof_collect(arr))
    finally:
        lib.mmnas_prof_enable(0)
        ops.BackboneFn.apply = orig_apply
        if sinks is not None:
            sinks.disable_sinks()
    if not arch:
        assert seen == [ragged], seen       # the chain was taken, on packed rows exactly when asked
    return seen


def _rows(path):
    rows = []
    for line in open(path).read().splitlines():
        kind, rest = line.split(',', 1)
        tag, _ms, flops, nbytes = rest.rsplit(',', 3)
        rows.append('%s,%s,%s,%s' % (kind, tag, flops, nbytes))
    return rows


@pytest.mark.parametrize('name', list(CONFIGS))
def test_chain_launch_schedule_equals_the_recorded_one(name, monkeypatch, tmp_path):
    import mmnas_amd._lib as L
    from mmnas_amd import ops
    step, setters, side, ragged = CONFIGS[name]
    lib = L.lib()
    dump = tmp_path / 'rows.csv'
    monkeypatch.setenv('MMNAS_PROF_DUMP', str(dump))
    monkeypatch.setenv('MMNAS_CHAIN', '1')
    monkeypatch.setenv('MMNAS_MIXED_CHAIN', '1')
    monkeypatch.setenv('MMNAS_SIDE_STREAM', side)
    prev = {}
    prev_unpad = ops.set_unpad(ragged)
    try:
        for k, v in setters.items():
            prev[k] = getattr(lib, 'mmnas_set_' + k)(v)
        _one_step(step, ragged)
    finally:
        for k, v in prev.items():
            getattr(lib, 'mmnas_set_' + k)(v)
        ops.set_unpad(prev_unpad)
    rows = _rows(str(dump))
    assert len(rows) > 50, len(rows)
    golden = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    if os.environ.get('MMNAS_REGEN_SCHEDULE') == '1':
        golden[name] = {'recorded_from': 'this change' if name in ONLY_THIS_CHANGE else 'parent commit', 'rows': rows}
        with open(GOLDEN, 'w') as f:
            json.dump({k: golden[k] for k in CONFIGS if k in golden}, f, indent=0)
            f.write('\n')
        return
    want = golden[name]
    assert (want['recorded_from'] == 'this change') == (name in ONLY_THIS_CHANGE)
    for n, (a, b) in enumerate(zip(rows, want['rows'])):
        assert a == b, 'launch %d of %s: issued %r, recorded %r' % (n, name, a, b)
    assert len(rows) == len(want['rows']), (name, len(rows), len(want['rows']), rows[len(want['rows']):][:3], want['rows'][len(rows):][:3])
