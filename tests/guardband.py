"""Guard bands around everything a kernel is handed: an `Arena` carves inputs, outputs, accumulators and scratch out of ONE
uint8 buffer, each as [band | payload | band], and `check()` then proves that the kernel wrote its outputs and nothing else.

  - the payload starts 256-byte aligned; the trailing band starts at the first byte behind the payload (no rounding in
    between: an overrun of one element lands in it);
  - a band is 4096 bytes: a condition, not a measurement -- four times the largest single store a wave issues (64 lanes x 16 B);
  - bands and row gaps of float tensors hold one quiet-NaN bit pattern (PATTERN) and are compared as int32, never as floats: an
    over-READ that reaches an accumulator shows as a NaN result, an over-WRITE as a changed word;
  - bands and gaps of integer / mask tensors (offset tables, indices, masks) hold zeros, so that an over-read index can never
    become a wild address through the test's own doing.

Works on any torch device (tests/test_guardband_host.py runs it on the CPU).  Plain module, not a conftest."""
import numpy as np
import torch

BAND = 4096
ALIGN = 256
PATTERN = 0x7FC5A17E                      # quiet NaN (exponent all ones, mantissa MSB set), mantissa reads "5A17E"
_PAT_I32 = int(np.array([PATTERN], dtype=np.uint32).view(np.int32)[0])
_PAT_BYTES = np.array([PATTERN], dtype='<u4').view(np.uint8)


class GuardBandError(AssertionError):
    pass


class _Rec:
    __slots__ = ('name', 'kind', 'off', 'nbytes', 'flat', 'view', 'shape', 'ld', 'width', 'rows', 'is_float', 'orig', 'written')


class Arena:
    def __init__(self, device, band_bytes=BAND, capacity=64 << 20):
        assert band_bytes % 4 == 0 and band_bytes > 0
        self.device = torch.device(device)
        self.band = int(band_bytes)
        self.buf = torch.empty(int(capacity) + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = (-self.buf.data_ptr()) % ALIGN     # buffer offset of the first aligned byte
        self.top = self.base                            # first free byte (always 4-byte aligned relative to base)
        self.recs = []

    # ------------------------------------------------------------------ layout
    def _fill(self, off, n, is_float):
        """Poison n bytes at buffer offset off: the pattern in phase with the ALIGNed grid (float) or zeros (integers)."""
        if n <= 0:
            return
        reg = self.buf[off:off + n]
        if not is_float:
            reg.zero_()
        elif (off - self.base) % 4 == 0 and n % 4 == 0:
            reg.view(torch.int32).fill_(_PAT_I32)
        else:
            idx = (np.arange(off - self.base, off - self.base + n) % 4)
            reg.copy_(torch.from_numpy(_PAT_BYTES[idx]).to(self.device))

    def _first_bad(self, off, n, is_float):
        """Index of the first byte of [off, off + n) that no longer holds its fill, or -1."""
        if n <= 0:
            return -1
        reg = self.buf[off:off + n]
        if not is_float:
            bad = reg != 0
            scale = 1
        elif (off - self.base) % 4 == 0 and n % 4 == 0:
            bad = reg.view(torch.int32) != _PAT_I32
            scale = 4
        else:
            idx = (np.arange(off - self.base, off - self.base + n) % 4)
            bad = reg != torch.from_numpy(_PAT_BYTES[idx]).to(self.device)
            scale = 1
        if not bool(bad.any()):
            return -1
        first = int(torch.nonzero(bad)[0, 0]) * scale
        if scale == 4:      # the byte inside the word
            word = reg[first:first + 4].cpu().numpy()
            first += int(np.nonzero(word != _PAT_BYTES)[0][0])
        return first

    def _carve(self, name, kind, dtype, shape, ld, nbytes=None):
        r = _Rec()
        r.name, r.kind = name or '%s%d' % (kind, len(self.recs)), kind
        r.is_float = dtype.is_floating_point
        item = torch.empty(0, dtype=dtype).element_size()
        if nbytes is None:
            shape = tuple(int(s) for s in shape)
            width = shape[-1] if shape else 1
            rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
            if ld is None or ld == width:
                ld = width
            assert ld >= width, (ld, width)
            numel = ((rows - 1) * ld + width) if rows and width else 0
            nbytes = numel * item
            r.shape, r.ld, r.width, r.rows = shape, ld, width, rows
        else:
            assert item == 1
            numel = int(nbytes)
            r.shape, r.ld, r.width, r.rows = (numel,), numel, numel, 1
        start = self.top + self.band
        start += (-(start - self.base)) % ALIGN
        end = start + nbytes
        if end + self.band > self.buf.numel():
            raise MemoryError('guard-band arena exhausted (%d bytes asked for %s)' % (nbytes, r.name))
        r.off, r.nbytes = start, nbytes
        self._fill(start - self.band, self.band, r.is_float)
        self._fill(end, self.band, r.is_float)
        self.top = end + self.band
        self.top += (-(self.top - self.base)) % 4
        raw = self.buf[start:end]
        r.flat = raw.view(dtype) if nbytes else torch.empty(0, dtype=dtype, device=self.device)
        if kind == 'scratch':
            r.view = r.flat
        elif r.ld == r.width:
            r.view = r.flat.view(r.shape)
        else:
            strides, s = [1], r.ld
            for n in reversed(r.shape[1:-1]):
                strides.insert(0, s)
                s *= n
            if len(r.shape) > 1:
                strides.insert(0, s)
            r.view = r.flat.as_strided(r.shape, strides)
        r.orig, r.written = None, None
        self.recs.append(r)
        return r

    # ------------------------------------------------------------------ the four calls
    def inp(self, array, ld=None, name=None):
        """Upload an input; with ld > width it is stored with that row stride and poisoned gaps.  -> (flat, view)"""
        t = torch.as_tensor(np.ascontiguousarray(array) if isinstance(array, np.ndarray) else array)
        r = self._carve(name, 'inp', t.dtype, t.shape if t.dim() else (1,), ld)
        self._fill(r.off, r.nbytes, r.is_float)
        r.view.copy_(t.reshape(r.shape).to(self.device))
        r.orig = self.buf[r.off:r.off + r.nbytes].clone()
        return r.flat, r.view

    def out(self, shape, ld=None, name=None, written=True):
        """An output pre-filled with the pattern.  `written`: True = every element must have been written; a boolean array of
        `shape` = exactly those elements are (the rest must still hold the pattern: the kernel's contract says it skips them)."""
        if isinstance(shape, int):
            shape = (shape,)
        r = self._carve(name, 'out', torch.float32, shape, ld)      # (an integer output: inout() of a sentinel value)
        self._fill(r.off, r.nbytes, r.is_float)
        r.written = written
        return r.flat, r.view

    def inout(self, array, ld=None, name=None):
        """A buffer the kernel accumulates into (or an integer output): uploaded, bands and gaps checked, contents free."""
        t = torch.as_tensor(np.ascontiguousarray(array) if isinstance(array, np.ndarray) else array)
        r = self._carve(name, 'inout', t.dtype, t.shape if t.dim() else (1,), ld)
        self._fill(r.off, r.nbytes, r.is_float)
        r.view.copy_(t.reshape(r.shape).to(self.device))
        return r.flat, r.view

    def scratch(self, nbytes, name=None):
        """A workspace of exactly nbytes, pre-filled with the pattern.  -> (uint8 flat view, the same view)"""
        r = self._carve(name, 'scratch', torch.uint8, None, None, nbytes=int(nbytes))
        r.is_float = True
        self._fill(r.off - self.band, self.band, True)
        self._fill(r.off, r.nbytes, True)
        self._fill(r.off + r.nbytes, self.band, True)
        return r.flat, r.view

    def scratch_floats(self, n, name=None):
        """scratch(4 n) as a float32 tensor (what a *_ws_floats() promise is handed as)."""
        flat, _ = self.scratch(4 * int(n), name)
        f = flat.view(torch.float32) if n else torch.empty(0, dtype=torch.float32, device=self.device)
        return f, f

    # ------------------------------------------------------------------ the verdict
    def _gap_bad(self, r):
        """First byte offset (from the payload start) inside a row gap that changed, or -1."""
        if r.ld == r.width or r.rows < 2:
            return -1
        iv = r.flat.view(torch.int32) if r.flat.element_size() == 4 else r.flat
        gaps = iv.as_strided((r.rows - 1, r.ld - r.width), (r.ld, 1), iv.storage_offset() + r.width)
        want = _PAT_I32 if r.is_float else 0
        assert not r.is_float or r.flat.element_size() == 4
        bad = gaps != want
        if not bool(bad.any()):
            return -1
        i, j = (int(v) for v in torch.nonzero(bad)[0])
        return (i * r.ld + r.width + j) * r.flat.element_size()

    def check(self):
        """Synchronise, then assert: every band and gap bitwise intact, every input bitwise what was uploaded, every output
        element written and finite.  The message names the tensor and the first offending byte offset (from the payload start:
        negative = leading band, >= payload bytes = trailing band)."""
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        for r in self.recs:
            b = self._first_bad(r.off + r.nbytes, self.band, r.is_float)
            if b >= 0:
                raise GuardBandError('%s: trailing band overwritten at payload byte offset %d (%d bytes past the %d-byte payload)'
                                     % (r.name, r.nbytes + b, b, r.nbytes))
            b = self._first_bad(r.off - self.band, self.band, r.is_float)
            if b >= 0:
                raise GuardBandError('%s: leading band overwritten at payload byte offset %d' % (r.name, b - self.band))
            if r.kind == 'scratch':
                continue
            b = self._gap_bad(r)
            if b >= 0:
                raise GuardBandError('%s: row gap overwritten at payload byte offset %d (row %d, ld %d, width %d)'
                                     % (r.name, b, b // (r.ld * r.flat.element_size()), r.ld, r.width))
            if r.kind == 'inp':
                bad = self.buf[r.off:r.off + r.nbytes] != r.orig
                if bool(bad.any()):
                    raise GuardBandError('%s: input modified at payload byte offset %d' % (r.name, int(torch.nonzero(bad)[0, 0])))
            if r.kind == 'out' and r.written is not None and r.flat.numel():
                item = r.flat.element_size()
                iv = r.flat.view(torch.int32).as_strided(r.view.shape, r.view.stride())
                unwritten = iv == _PAT_I32
                if r.written is True:
                    must = torch.ones_like(unwritten)
                else:
                    must = torch.from_numpy(np.array(r.written, dtype=bool)).reshape(r.shape).to(self.device)
                    stray = ~must & ~unwritten
                    if bool(stray.any()):
                        raise GuardBandError('%s: element the contract leaves alone was written at payload byte offset %d'
                                             % (r.name, self._elem_off(r, stray) * item))
                miss = must & unwritten
                if bool(miss.any()):
                    raise GuardBandError('%s: output element not written at payload byte offset %d' % (r.name, self._elem_off(r, miss) * item))
                nonfin = must & ~torch.isfinite(r.view)
                if bool(nonfin.any()):
                    raise GuardBandError('%s: output element not finite at payload byte offset %d' % (r.name, self._elem_off(r, nonfin) * item))

    @staticmethod
    def _elem_off(r, mask):
        idx = [int(v) for v in torch.nonzero(mask)[0]]
        return sum(i * s for i, s in zip(idx, r.view.stride()))
