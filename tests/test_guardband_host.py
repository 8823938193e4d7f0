"""tests/guardband.py fails when it should (CPU): one float just past a payload, just before it, in a row gap; one flipped
input element; one unwritten output element; a scratch buffer overrun by 4 bytes -- each raises and names the tensor and the
offset.  A clean run passes.  Payload starts are aligned and the trailing band starts at payload_end exactly."""
import numpy as np
import pytest
import torch

from tests.guardband import ALIGN, BAND, PATTERN, Arena, GuardBandError


def _setup():
    """What one kernel call is handed: a strided input, an index table, a strided output, an accumulator, scratch."""
    rs = np.random.RandomState(0)
    ar = Arena('cpu')
    x = rs.standard_normal((5, 7)).astype(np.float32)
    t = {'x': ar.inp(x, ld=11, name='x'),
         'idx': ar.inp(np.arange(6, dtype=np.int32), name='idx'),
         'mask': ar.inp(np.array([[0, 1, 1]], dtype=np.uint8), name='mask'),
         'y': ar.out((5, 7), ld=9, name='y'),
         'acc': ar.inout(np.zeros(3, np.float32), name='acc'),
         'ws': ar.scratch(100, name='ws')}
    t['y'][1].copy_(torch.from_numpy(x) * 2)          # the "kernel": writes exactly its output
    t['acc'][1].add_(1.0)
    t['ws'][0][:100] = 7
    return ar, t, x


def _past(ar, name, byte_off, value=1.0):
    """Store one float at `byte_off` bytes from the payload start of tensor `name`, straight into the arena's buffer."""
    r = [r for r in ar.recs if r.name == name][0]
    ar.buf[r.off + byte_off:r.off + byte_off + 4].view(torch.float32).fill_(value)


def test_clean_run_passes_and_reads_back():
    ar, t, x = _setup()
    ar.check()
    assert np.array_equal(t['y'][1].numpy(), x * 2) and np.array_equal(t['x'][1].numpy(), x)
    assert t['x'][0].is_contiguous() and t['x'][0].dim() == 1 and t['x'][0].numel() == 4 * 11 + 7
    assert t['x'][1].stride() == (11, 1) and t['y'][1].stride() == (9, 1)


def test_layout_alignment_and_band_position():
    ar, t, _ = _setup()
    prev_end = None
    for r in ar.recs:
        assert (ar.buf.data_ptr() + r.off) % ALIGN == 0, r.name
        assert r.flat.data_ptr() == ar.buf.data_ptr() + r.off or r.nbytes == 0
        if prev_end is not None:
            assert r.off - BAND >= prev_end, 'bands of neighbouring tensors overlap'
        prev_end = r.off + r.nbytes + BAND
        # the trailing band starts at the first byte behind the payload: no rounding in between
        tail = ar.buf[r.off + r.nbytes:r.off + r.nbytes + BAND]
        lead = ar.buf[r.off - BAND:r.off]
        if r.is_float:
            want = np.array([PATTERN], dtype='<u4').view(np.uint8)
            phase = np.arange(r.nbytes, r.nbytes + BAND) % 4
            assert np.array_equal(tail.numpy(), want[phase]), r.name
            assert np.array_equal(lead.numpy(), np.tile(want, BAND // 4)), r.name
        else:
            assert not tail.any() and not lead.any(), r.name
    ws = [r for r in ar.recs if r.name == 'ws'][0]
    assert ws.nbytes == 100 and t['ws'][0].numel() == 100
    # float bands read back as NaN, index bands as zero
    xr = [r for r in ar.recs if r.name == 'x'][0]
    assert torch.isnan(ar.buf[xr.off + xr.nbytes:xr.off + xr.nbytes + 4].view(torch.float32)).all()
    assert torch.isnan(t['x'][0][7:11]).all()        # a row gap


@pytest.mark.parametrize('name,off,what', [    # (off: where the float 1.0 = bytes 00 00 80 3f is stored)
    ('y', (4 * 9 + 7) * 4, 'trailing band'),           # one float just past the payload
    ('y', -4, 'leading band'),                         # one float just before it
    ('y', (2 * 9 + 8) * 4, 'row gap'),                 # into a row gap (row 2, column 8 of ld 9)
    ('x', (4 * 11 + 7) * 4, 'trailing band'),
    ('x', 7 * 4, 'row gap'),
    ('acc', 12, 'trailing band'),
    ('idx', 24, 'trailing band'),
    ('ws', 100, 'trailing band'),                      # scratch overrun by 4 bytes
])
def test_stray_store_is_reported(name, off, what):
    ar, _, _ = _setup()
    _past(ar, name, off)
    with pytest.raises(GuardBandError) as e:
        ar.check()
    msg = str(e.value)
    first = off + 2 if name == 'idx' else off       # zero-filled integer bands: the first two bytes of 1.0 are zero
    assert msg.startswith(name + ':') and what in msg and ('offset %d' % first) in msg, msg


def test_bands_are_compared_bit_for_bit():
    """A NaN with another mantissa than the pattern's is a violation like any other value."""
    ar, _, _ = _setup()
    _past(ar, 'y', (4 * 9 + 7) * 4 + 64, value=float('nan'))     # torch's NaN: another bit pattern
    with pytest.raises(GuardBandError, match=r'y: trailing band .* offset %d ' % ((4 * 9 + 7) * 4 + 64)):
        ar.check()


def test_flipped_input_element_is_reported():
    ar, t, _ = _setup()
    t['x'][1][3, 2] = -t['x'][1][3, 2]
    with pytest.raises(GuardBandError) as e:
        ar.check()
    # the sign bit: the last byte of the little-endian word
    assert str(e.value) == 'x: input modified at payload byte offset %d' % ((3 * 11 + 2) * 4 + 3)
    ar, t, _ = _setup()
    t['mask'][1][0, 1] = 0
    with pytest.raises(GuardBandError, match='mask: input modified at payload byte offset 1$'):
        ar.check()


def test_unwritten_and_non_finite_output_elements_are_reported():
    ar, t, _ = _setup()
    _past(ar, 'y', (3 * 9 + 6) * 4, value=0.0)
    ar.check()                                        # (any written value passes)
    ar.buf[[r for r in ar.recs if r.name == 'y'][0].off + (3 * 9 + 6) * 4:][:4].view(torch.int32).fill_(
        int(np.array([PATTERN], np.uint32).view(np.int32)[0]))
    with pytest.raises(GuardBandError, match='y: output element not written at payload byte offset %d$' % ((3 * 9 + 6) * 4)):
        ar.check()
    ar, t, _ = _setup()
    t['y'][1][0, 1] = float('inf')
    with pytest.raises(GuardBandError, match='y: output element not finite at payload byte offset 4$'):
        ar.check()


def test_partial_output_contract():
    """written = a mask: exactly those elements are written, the others still hold the pattern."""
    ar = Arena('cpu', band_bytes=64)
    must = np.zeros((3, 4), bool)
    must[:2, :3] = True
    _, y = ar.out((3, 4), name='part', written=must)
    y[:2, :3] = 1.0
    ar.check()
    y[2, 0] = 1.0
    with pytest.raises(GuardBandError, match='part: element the contract leaves alone was written at payload byte offset 32$'):
        ar.check()


def test_empty_payloads_and_exhaustion():
    ar = Arena('cpu', capacity=6 * BAND)
    f, v = ar.scratch(0, name='none')
    assert f.numel() == 0
    e, _ = ar.inp(np.zeros((0, 4), np.float32), name='empty')
    assert e.numel() == 0
    ar.check()
    with pytest.raises(MemoryError):
        ar.out((1 << 20,), name='big')
