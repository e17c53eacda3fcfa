"""Guard bands around what the kernels read and write (tests/test_gpu_guard_bands.py; tested itself, on CPU tensors, by
tests/test_guard_bands_host.py).

An `Arena` hands out float64 arrays embedded in larger allocations of its own, [guard | payload | guard]:

* each guard is at least max(64 KiB, the payload's size), so that a store window one whole trial -- or one whole 64-trial block -- too long
  still lands in memory the test owns: the test never makes a stray access leave allocated memory;
* `placement='aligned'` puts the payload on a multiple of 256 bytes (what torch's allocator hands out), `'odd'` on an address that is
  8 (mod 16) -- all the C-ABI asks of a caller's float64 array;
* guards hold one quiet-NaN bit pattern (GUARD), output payloads are pre-filled with a second one (PREFILL).  No arithmetic produces
  either and both differ from the canonical NaN 0x7FF8000000000000, so a word that still holds PREFILL was never written, whatever was
  computed for it -- NaN included.  Everything is compared as int64.

`check()` lists (a) every run of guard words that changed -- array, side, byte distance from the payload -- and (b) every output word
that still holds PREFILL.  `installed()` makes the arena the allocator of chirpgp_amd._engine's outputs (_engine._new_output) for the
length of a `with` block."""
import contextlib

import numpy as np

GUARD = 0x7FFA5A5A5A5A5A5A             # sign 0, exponent all ones, quiet bit, payload 0x25A5A5A5A5A5A
PREFILL = 0x7FFC3C3C3C3C3C3C
CANONICAL_NAN = 0x7FF8000000000000
MIN_GUARD_BYTES = 64 * 1024
PLACEMENTS = ('aligned', 'odd')
_SLACK = 32                            # words: room to move the payload onto the next 256-byte boundary


def guard_words(payload_words):
    """Words in each guard of a payload of that many words: max(64 KiB, the payload's own size)."""
    return max(MIN_GUARD_BYTES // 8, int(payload_words))


class _Block:
    def __init__(self, name, kind, words, offset, n, shape):
        self.name, self.kind, self.words, self.offset, self.n, self.shape = name, kind, words, offset, n, shape

    @property
    def payload(self):
        return self.words[self.offset:self.offset + self.n]

    @property
    def guards(self):
        return (('front', self.words[:self.offset]), ('back', self.words[self.offset + self.n:]))


class Arena:
    def __init__(self, device, placement):
        import torch
        if placement not in PLACEMENTS:
            raise ValueError(f'placement must be one of {PLACEMENTS}')
        self.torch, self.device, self.placement = torch, torch.device(device), placement
        self.blocks = []
        self.requests = []             # (name, shape) of every output asked for, in order

    # ---- allocation
    def _embed(self, name, kind, shape, placement=None):
        torch = self.torch
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        g = guard_words(n)
        words = torch.full((g + _SLACK + n + g,), GUARD, dtype=torch.int64, device=self.device)
        base = words.data_ptr()
        assert base % 8 == 0
        offset = g + (-(base + 8 * g) % 256) // 8                # the payload on a multiple of 256 ...
        if (placement or self.placement) == 'odd':
            offset += 1                                          # ... or one double behind it: 8 (mod 16)
        block = _Block(name, kind, words, offset, n, shape)
        self.blocks.append(block)
        return block

    def output(self, shape, name=None, placement=None):
        """A contiguous float64 view of `shape` pre-filled with PREFILL, for a kernel to write."""
        name = name or f'output{len(self.requests)}'
        self.requests.append((name, tuple(int(s) for s in shape)))
        block = self._embed(name, 'output', shape, placement)
        block.payload.fill_(PREFILL)
        return block.payload.view(self.torch.float64).view(block.shape)

    def input(self, array, name=None, placement=None):
        """A copy of `array` (NumPy or torch, any float dtype) between guards that hold GUARD: what a kernel reads beyond it is NaN."""
        torch = self.torch
        t = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(array, dtype=np.float64)))
        t = t.to(torch.float64).contiguous()
        block = self._embed(name or f'input{len(self.blocks)}', 'input', tuple(t.shape), placement)
        view = block.payload.view(torch.float64).view(block.shape)
        view.copy_(t.to(self.device))
        return view

    def _seam(self, shape, device, name=None):
        assert self.torch.device(device).type == self.device.type, (device, self.device)
        return self.output(shape, name)

    @contextlib.contextmanager
    def installed(self):
        """The arena as _engine._new_output inside the block; the allocator that was there comes back afterwards, whatever happens."""
        from chirpgp_amd import _engine
        before = _engine._new_output
        _engine._new_output = self._seam
        try:
            yield self
        finally:
            _engine._new_output = before

    # ---- inspection
    def guard_violations(self, limit=8):
        """Runs of changed guard words: '<name> <side> guard: <n> words changed, <first> .. <last> bytes <before|behind> the payload'."""
        found = []
        for b in self.blocks:
            for side, words in b.guards:
                bad = (words != GUARD).nonzero().reshape(-1).cpu().numpy()
                if bad.size == 0:
                    continue
                # byte distance of a word's first byte from the payload's nearest edge: 8 for the word next to it
                dist = (b.offset - bad) * 8 if side == 'front' else (bad + 1) * 8
                found.append(f'{b.name} {b.shape} {side} guard: {bad.size} words changed, {int(dist.min())} .. {int(dist.max())} bytes '
                             f'{"before" if side == "front" else "behind"} the payload; first at distances {sorted(int(v) for v in dist)[:limit]}')
        return found

    def unwritten(self, limit=8):
        """Output words that still hold PREFILL: '<name> <shape>: <n> of <N> words never written, first at <indices>'."""
        found = []
        for b in self.blocks:
            if b.kind != 'output':
                continue
            bad = (b.payload == PREFILL).nonzero().reshape(-1).cpu().numpy()
            if bad.size:
                where = [tuple(int(i) for i in np.unravel_index(int(k), b.shape)) for k in bad[:limit]]
                found.append(f'{b.name} {b.shape}: {bad.size} of {b.n} words never written, first at {where}')
        return found

    def written(self):
        """(name, number of words that no longer hold PREFILL) of every output that was touched at all -- empty after a refused call."""
        out = []
        for b in self.blocks:
            if b.kind == 'output':
                n = int((b.payload != PREFILL).sum())
                if n:
                    out.append((b.name, n))
        return out

    def check(self):
        """Every violation: guard words that changed, output words never written.  Empty: the launch wrote all of its outputs, nothing else."""
        if self.device.type == 'cuda':
            self.torch.cuda.synchronize(self.device)
        return self.guard_violations() + self.unwritten()


def same_bits(a, b):
    """Two float64 tensors (or None twice) equal bit for bit, NaN payloads included."""
    import torch
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))
