"""Cost tables of the hardware-aware architecture search: one figure per candidate operator, laid out as the
[nodes, width] block the fused alpha update reads (ops.alpha_cost_step, harness.ArchAdam(cost=...)).

A block's rows are `net.redundant_modules`, its columns each node's `Used_OPS`, padding columns hold 0.  The figures are
either algorithmic flops (flop_cost_table: no measurement needed) or whatever a CostTable file carries --
tools/op_cost_table.py writes one with the measured forward + backward time of every candidate on the MI355X.
"""
import json
import math

import torch

from .model.mixed import MixedOp


_NAMES = None


def _registry():
    global _NAMES
    if _NAMES is None:
        from .utils.ops_adapter import OpsAdapter
        _NAMES = frozenset(OpsAdapter().OPS)
    return _NAMES


def _att_flops(S, Skv, d, di):
    # q and merge projections over the S query rows, k and v over the Skv key rows, QK^T and PV
    return 4 * S * d * di + 4 * Skv * d * di + 4 * S * Skv * di


def op_flops(name, cfg, Sx, Sy, kind):
    """Algorithmic forward flops (a multiply-add counts two; elementwise work, softmax and LayerNorm are not counted) of the
    registry operator `name` for ONE sample: `kind` 'enc' runs on the Sx-token stream, 'dec' on the Sy-region stream with the
    encoder's Sx rows as the second input.  For the shipped search spaces this is bench.py's op_flops_fwd at B = 1."""
    if kind not in ('enc', 'dec'):
        raise ValueError("op_flops: kind is 'enc' or 'dec', got %r" % (kind,))
    if name not in _registry():
        raise ValueError('op_flops: %r is not a registry operator' % (name,))
    d = cfg.HSIZE
    S = Sx if kind == 'enc' else Sy
    if name in ('none', 'skip_connect', 'relu', 'gelu', 'leakyrelu'):
        return 0
    part = name.split('_')
    if 'att' in part:
        at = part.index('att')
        base = int(part[at + 1])
        di = d * int(part[at + 2]) if len(part) > at + 2 else d       # 'self_att_64_2': hsize_k = 2
        if name.startswith('guided_att_'):
            return _att_flops(S, Sx, d, di)
        if name.startswith('uniimg_att_'):
            return _att_flops(S, S + Sx, d, di)                         # k = v = cat(x, y)
        if name.startswith('rel_self_att_'):
            return _att_flops(S, S, d, di) + 2 * S * S * getattr(cfg, 'REL_SIZE', 64) * (di // base)
        if name.startswith('self_att_'):
            return _att_flops(S, S, d, di)
    if name == 'feed_forward':
        return 16 * S * d * d
    if name == 'feed_forward_deep':                                     # d -> 2d -> 2d -> d
        return 16 * S * d * d
    if name.startswith('feed_forward_'):
        return 4 * S * d * d * int(part[-1])                            # mid = mid_k * d
    if name == 'gated_linear_1':                                        # d -> 2d, gated to d
        return 4 * S * d * d
    if name == 'gated_linear_2':                                        # d -> 4d gated to 2d, 2d -> 2d gated to d
        return 16 * S * d * d
    if name.startswith('sep_conv_'):
        return 2 * S * d * int(part[-1]) + 2 * S * d * d
    if name.startswith('std_conv_'):
        return 2 * S * d * d * int(part[-1])
    raise ValueError('op_flops: no formula for the registry operator %r' % (name,))


def node_kinds(net):
    """'enc' / 'dec' per MixedOp, in the order of net.redundant_modules."""
    kinds = ['enc' if 'cells_enc' in n else 'dec' for n, m in net.named_modules() if isinstance(m, MixedOp)]
    if len(kinds) != len(net.redundant_modules):
        raise ValueError('node_kinds: %d named MixedOps, %d redundant modules' % (len(kinds), len(net.redundant_modules)))
    return kinds


def _block(net, figure):
    mods = net.redundant_modules
    width = max(m.n_choices for m in mods)
    block = torch.zeros(len(mods), width, dtype=torch.float32)
    for i, (m, kind) in enumerate(zip(mods, node_kinds(net))):
        for j, name in enumerate(m.Used_OPS):
            block[i, j] = figure(name, kind)
    return block


def flop_cost_table(net, Sx, Sy, unit=1e6):
    """[nodes, width] float32: op_flops of every candidate of every node in units of `unit` flops (default MFLOP)."""
    return _block(net, lambda name, kind: op_flops(name, net._cfg, Sx, Sy, kind) / unit)


def check_block(block, n_choices=None, cost_form='linear'):
    """What the alpha update asks of a cost block: finite, not negative, 0 in the padding columns; for the 'log' form (which
    divides by the expected cost) at least one positive entry."""
    if not bool(torch.isfinite(block).all()) or bool((block < 0).any()):
        raise ValueError('cost block: every cost is finite and not negative')
    if n_choices is not None:
        for i, n in enumerate(n_choices):
            if bool((block[i, n:] != 0).any()):
                raise ValueError('cost block: row %d holds a cost in a padding column (node has %d candidates)' % (i, n))
    if cost_form == 'log' and not bool((block > 0).any()):
        raise ValueError("cost block: cost_form='log' needs at least one positive cost")
    return block


def uniform_expected(block, n_choices):
    """Sum over the nodes of the mean cost over the node's live candidates: the expected cost under uniform alphas, the
    default cost_ref."""
    return float(sum(float(block[i, :n].double().mean()) for i, n in enumerate(n_choices)))


class CostTable:
    """One cost per candidate name and stream: enc / dec {name: cost}, `unit` a label ('us', 'MFLOP', ...), `meta` whatever the
    producer wants to keep beside the figures (shapes, runtime configuration, raw timings)."""

    def __init__(self, enc, dec, unit='', meta=None):
        self.enc, self.dec = dict(enc), dict(dec)
        self.unit, self.meta = unit, dict(meta or {})
        for kind, tab in (('enc', self.enc), ('dec', self.dec)):
            for name, c in tab.items():
                if not isinstance(c, (int, float)) or not math.isfinite(c) or c < 0:
                    raise ValueError('CostTable: %s[%r] = %r: a cost is a finite number, not negative' % (kind, name, c))

    def to_json(self, path):
        with open(path, 'w') as f:
            json.dump({'unit': self.unit, 'enc': self.enc, 'dec': self.dec, 'meta': self.meta}, f, indent=1, sort_keys=True)
            f.write('\n')

    @classmethod
    def from_json(cls, path):
        with open(path) as f:
            d = json.load(f)
        return cls(d['enc'], d['dec'], unit=d.get('unit', ''), meta=d.get('meta'))

    def _figure(self, name, kind):
        tab = self.enc if kind == 'enc' else self.dec
        if name not in tab:
            raise ValueError('CostTable: no %s cost for candidate %r' % (kind, name))
        return float(tab[name])

    def for_net(self, net, cost_form='linear'):
        """The [nodes, width] float32 block for `net` (on the CPU); ValueError for a candidate the table does not name and,
        with cost_form='log', for a table without a positive entry."""
        return check_block(_block(net, self._figure), [m.n_choices for m in net.redundant_modules], cost_form)

    def uniform_expected(self, net):
        return uniform_expected(self.for_net(net), [m.n_choices for m in net.redundant_modules])
