"""The drop-in import surface: with this repository on the path next to an integrator's checkout of the
reference, every `from mmnas... import ...` line of the six entry scripts resolves -- the operator hot path
(`mmnas.model.*`, `mmnas.utils.{ops_adapter,optimizer,itm_loss}`) to THIS tree, everything else (`mmnas.loader.*`,
`mmnas.utils.{sampler,vqa,vqaEval,bbox_transform,bbox}`: out of scope) to the checkout.  The checkout is rebuilt in a
temporary directory from the scripts' recorded import lines (tests/golden/entry_imports.json).  Child interpreters,
because the test process itself has `mmnas` imported already."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OURS = {'mmnas.model.hygr_vqa', 'mmnas.model.hygr_vgd', 'mmnas.model.hygr_itm', 'mmnas.model.full_vqa', 'mmnas.model.full_vgd',
        'mmnas.model.full_itm', 'mmnas.model.mixed', 'mmnas.model.modules', 'mmnas.utils.ops_adapter', 'mmnas.utils.optimizer',
        'mmnas.utils.itm_loss'}

CHILD = r'''
import importlib, importlib.util, json, re, sys
script_dir, scripts = sys.argv[1], sys.argv[2:]
if script_dir:
    sys.path.insert(0, script_dir)          # what `python3 search_vqa.py` run from the checkout has as sys.path[0]
out = {}
for s in scripts:
    for ln, line in enumerate(open(s), 1):
        m = re.match(r'from (mmnas[\w.]*) import (.+)', line)
        if not m:
            continue
        mod, names = m.group(1), [n.strip() for n in m.group(2).split(',')]
        try:
            spec = importlib.util.find_spec(mod)
            parent_path = list(importlib.import_module(mod.rsplit('.', 1)[0]).__path__)
        except ModuleNotFoundError:          # the parent package itself is absent
            spec, parent_path = None, []
        rec = {'origin': spec.origin if spec else None, 'names': names, 'missing': None, 'import_error': None, 'parent_path': parent_path}
        try:
            mm = importlib.import_module(mod)
            rec['missing'] = [n for n in names if not hasattr(mm, n)]
        except Exception as e:
            rec['import_error'] = '%s: %s' % (type(e).__name__, e)
        out['%s:%d %s' % (s.rsplit('/', 1)[-1], ln, mod)] = rec
print(json.dumps(out))
'''


def _resolve(env_extra, cwd, script_dir, scripts):
    env = {k: v for k, v in os.environ.items() if k not in ('PYTHONPATH', 'MMNAS_REFERENCE_ROOT')}
    env.update(env_extra, PYTHONDONTWRITEBYTECODE='1')
    p = subprocess.run([sys.executable, '-c', CHILD, script_dir] + scripts, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _checkout_tree(co):
    """A tree shaped like the reference checkout, from the import surface of its six entry scripts
    (tests/golden/entry_imports.json, written by make_golden.gen_entry_imports): the scripts as their `from mmnas...`
    lines; every out-of-scope module they import as a stub defining the imported names; the operator modules this tree
    must shadow as files that raise when imported; the Cython module as its unbuilt .pyx source only."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'entry_imports.json')) as f:
        surface = json.load(f)
    names = {}
    for rows in surface['scripts'].values():
        for _, mod, ns in rows:
            names.setdefault(mod, set()).update(ns)
    for mod, ns in names.items():
        path = co.joinpath(*mod.split('.'))
        path.parent.mkdir(parents=True, exist_ok=True)       # (no __init__.py: the checkout's mmnas is a namespace package)
        if mod in surface['cython_only']:
            path.with_suffix('.pyx').write_text('# unbuilt Cython source\n')
        elif mod in OURS:
            path.with_suffix('.py').write_text('raise RuntimeError("the checkout\'s %s must be shadowed")\n' % mod)
        else:
            path.with_suffix('.py').write_text(''.join('class %s:\n    pass\n' % n for n in sorted(ns)))
    scripts = []
    for s, rows in sorted(surface['scripts'].items()):
        lines = [''] * max(ln for ln, _, _ in rows)          # each import on its line number in the script
        for ln, mod, ns in rows:
            lines[ln - 1] = 'from %s import %s' % (mod, ', '.join(ns))
        (co / s).write_text('\n'.join(lines) + '\n')
        scripts.append(str(co / s))
    return scripts, set(surface['cython_only']), sum(len(rows) for rows in surface['scripts'].values())


@pytest.mark.parametrize('how', ['script_dir_first', 'pythonpath_pair', 'reference_root_variable'])
def test_every_mmnas_import_of_the_entry_scripts_resolves_to_the_expected_tree(how, tmp_path):
    ref = tmp_path / 'checkout'
    scripts, cython_only, n_lines = _checkout_tree(ref)
    REF = str(ref)
    run_dir = tmp_path / 'elsewhere'
    run_dir.mkdir()
    if how == 'script_dir_first':        # `cd <checkout>; PYTHONPATH=<repo> python3 search_vqa.py`
        got = _resolve({'PYTHONPATH': ROOT}, REF, REF, scripts)
    elif how == 'pythonpath_pair':       # PYTHONPATH=<repo>:<checkout>
        got = _resolve({'PYTHONPATH': ROOT + os.pathsep + REF}, str(run_dir), '', scripts)
    else:                                # checkout not on the path at all
        got = _resolve({'PYTHONPATH': ROOT, 'MMNAS_REFERENCE_ROOT': REF}, str(run_dir), '', scripts)
    assert len(got) == n_lines == 43     # the import lines listed in search_vqa.py:17-24, train_vgd.py:15-21, search_itm.py:17-23, ...
    seen_ref = set()
    for key, r in got.items():
        mod = key.split()[-1]
        if mod in cython_only:
            # the checkout's Cython module (mmnas/utils/bbox.pyx + setup.py), unbuilt here: the directory it is built
            # into must be on the package's search path
            assert r['origin'] is None, (key, r)
            assert os.path.join(REF, 'mmnas', 'utils') in r['parent_path'] and os.path.exists(os.path.join(REF, 'mmnas', 'utils', 'bbox.pyx'))
            seen_ref.add(mod)
            continue
        assert r['origin'], key
        if mod in OURS:
            assert r['origin'].startswith(ROOT + os.sep), (key, r['origin'])
            assert r['import_error'] is None and r['missing'] == [], (key, r)      # e.g. Margin_Loss (search_itm.py:23)
        else:
            assert r['origin'].startswith(REF + os.sep), (key, r['origin'])
            assert r['import_error'] is None and r['missing'] == [], (key, r)
            seen_ref.add(mod)
    assert {'mmnas.loader.filepath_vqa', 'mmnas.loader.load_data_vqa', 'mmnas.utils.sampler', 'mmnas.utils.vqa', 'mmnas.utils.vqaEval',
            'mmnas.utils.bbox_transform', 'mmnas.utils.bbox'} <= seen_ref


def test_alias_package_next_to_a_checkout_shaped_tree(tmp_path):
    """The same mechanism without the reference (runs anywhere): a tree shaped like the checkout's namespace package."""
    co = tmp_path / 'checkout'
    (co / 'mmnas' / 'loader').mkdir(parents=True)
    (co / 'mmnas' / 'utils').mkdir()
    (co / 'mmnas' / 'model').mkdir()
    (co / 'mmnas' / 'loader' / 'filepath_vqa.py').write_text('class Path: pass\n')
    (co / 'mmnas' / 'utils' / 'sampler.py').write_text('class SubsetDistributedSampler: pass\n')
    (co / 'mmnas' / 'utils' / 'optimizer.py').write_text('raise RuntimeError("the checkout\'s optimizer must be shadowed")\n')
    (co / 'mmnas' / 'model' / 'mixed.py').write_text('raise RuntimeError("the checkout\'s operators must be shadowed")\n')
    script = co / 'entry.py'
    script.write_text('from mmnas.loader.filepath_vqa import Path\nfrom mmnas.utils.sampler import SubsetDistributedSampler\n'
                      'from mmnas.utils.optimizer import WarmupOptimizer\nfrom mmnas.model.mixed import MixedOp\n'
                      'from mmnas.utils.itm_loss import BCE_Loss, Margin_Loss\n')
    for env, sd in (({'PYTHONPATH': ROOT}, str(co)), ({'PYTHONPATH': ROOT + os.pathsep + str(co)}, ''),
                    ({'PYTHONPATH': str(co) + os.pathsep + ROOT}, ''), ({'PYTHONPATH': ROOT, 'MMNAS_REFERENCE_ROOT': str(co)}, '')):
        got = _resolve(env, str(tmp_path), sd, [str(script)])
        assert len(got) == 5
        for key, r in got.items():
            mod = key.split()[-1]
            want = ROOT if mod in OURS else str(co)
            assert r['origin'].startswith(want + os.sep) and r['import_error'] is None and r['missing'] == [], (env, key, r)
    # without any checkout the out-of-scope modules are simply absent (no half-resolved package)
    got = _resolve({'PYTHONPATH': ROOT}, str(tmp_path), '', [str(script)])
    assert [k.split()[-1] for k, r in got.items() if r['origin'] is None] == ['mmnas.loader.filepath_vqa', 'mmnas.utils.sampler']


def test_margin_loss_closed_form():
    """mmnas/utils/itm_loss.py:27-37."""
    import numpy as np
    import torch
    from mmnas.utils.itm_loss import Margin_Loss
    g = torch.Generator().manual_seed(3)
    sp, sc, si = (torch.rand(17, 1, generator=g, requires_grad=True) for _ in range(3))
    loss = Margin_Loss(None)(sp, sc, si)
    a, b, c = (t.detach().numpy().astype(np.float64) for t in (sp, sc, si))
    want = np.maximum(0.2 + b - a, 0).sum() + np.maximum(0.2 + c - a, 0).sum()
    assert abs(float(loss.detach()) - want) < 1e-5
    loss.backward()
    gp = -((0.2 + b - a) > 0).astype(np.float64) - ((0.2 + c - a) > 0).astype(np.float64)
    assert np.allclose(sp.grad.numpy(), gp) and np.allclose(sc.grad.numpy(), ((0.2 + b - a) > 0))
