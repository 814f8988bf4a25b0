"""Guard bands for caller-owned buffers — TEST INFRASTRUCTURE ONLY (a plain module like clip_ref.py).

include/spwgnn.h states a memory contract for every entry point: outputs are written in full and nothing
past them, inputs are const, a workspace of exactly spwgnn_workspace_bytes() is enough. torch's caching
allocator hides a violation: it rounds every allocation up to 512 B and carves small tensors out of shared
segments, so a store one row past an output lands in slack or in some other tensor. An `Arena` hands out
tensors that sit in the middle of its own buffers instead:

    | ... BAND bytes of 0xA5 ... | payload | ... BAND bytes of 0xA5 ... |

  * BAND = 64 KiB: more than the largest overrun a 128-row workgroup tile of 100-float rows could make
    (51,200 B), so an overrun of that class lands in a band, not in unmapped memory.
  * The payload starts at an address that is a multiple of the requested alignment and NOT of twice that:
    a kernel that needs more alignment than the header asks for does not get it by accident.
  * An output (`alloc(..., written=True)`) is pre-filled with the "unwritten" pattern 0xC3C3C3C3, a finite
    float (−391.53), so an unwritten element is found by its bits and poisons nothing on the way.
  * `freeze(t)` registers an input and keeps a clone.

`check()` synchronises and asserts, naming the buffer: every band byte is still the sentinel; no element of
a `written` output still holds the unwritten pattern (compared as int32); every frozen input equals its
clone bit for bit. Works on CPU tensors too (tests/test_guard_host.py)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

BAND = 64 * 1024
SENTINEL = 0xA5                      # every byte of a band
UNWRITTEN = 0xC3                     # every byte of an output before the call
UNWRITTEN_I32 = int(np.array([0xC3C3C3C3], np.uint32).view(np.int32)[0])
CHUNK = 8 << 20                      # backing buffers are at least this large


@dataclass
class _Alloc:
    name: str
    chunk: int          # index of the backing buffer
    start: int          # payload's byte offset in it
    nbytes: int
    view: torch.Tensor
    written: bool
    frozen: Optional[torch.Tensor] = None


class _Chunk:
    """A backing buffer. A shared one keeps a byte mask of its bands (one comparison checks them all); a
    request too large to share (a workspace) gets a buffer of its own whose two bands are sliced instead."""

    def __init__(self, nbytes: int, device, solo: bool):
        self.buf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=device)
        self.band = None if solo else torch.ones(nbytes, dtype=torch.bool, device=device)   # False over the payloads
        self.used = 0

    def damaged(self, allocs) -> Optional[torch.Tensor]:
        """Sorted backing offsets of the band bytes that no longer hold the sentinel, or None."""
        if self.band is not None:
            bad = (self.buf != SENTINEL) & self.band
            return torch.nonzero(bad).reshape(-1) if bool(bad.any()) else None
        (a,) = allocs
        end = a.start + a.nbytes
        lead, trail = self.buf[:a.start] != SENTINEL, self.buf[end:] != SENTINEL
        if not bool(lead.any()) and not bool(trail.any()):
            return None
        return torch.cat([torch.nonzero(lead).reshape(-1), torch.nonzero(trail).reshape(-1) + end])


class Arena:
    def __init__(self, device):
        self.device = torch.device(device)
        self.chunks: list[_Chunk] = []
        self.allocs: list[_Alloc] = []
        self._shared: Optional[int] = None   # the shared backing buffer that is being filled

    # ------------------------------------------------------------------------------ allocation
    def _place(self, nbytes: int, align: int):
        """(chunk index, payload offset): BAND bytes after the previous payload (or the chunk's start),
        moved up to an address that is a multiple of `align` and an odd one."""
        need = BAND + 2 * align + nbytes + BAND
        if need > CHUNK:
            self.chunks.append(_Chunk(need, self.device, solo=True))
            ci = len(self.chunks) - 1
        else:
            ci = self._shared
            if ci is None or self.chunks[ci].used + need > self.chunks[ci].buf.numel():
                self.chunks.append(_Chunk(CHUNK, self.device, solo=False))
                ci = self._shared = len(self.chunks) - 1
        c = self.chunks[ci]
        base = c.buf.data_ptr()
        addr = base + c.used + BAND
        addr = (addr + align - 1) // align * align
        if addr % (2 * align) == 0:
            addr += align
        start = addr - base
        c.used = start + nbytes          # the next payload's leading band is this one's trailing band
        return ci, start

    def alloc(self, shape, dtype, align: int = 16, name: str = "?", written: bool = False) -> torch.Tensor:
        """A contiguous view of `shape` between two bands. `written`: an output the call must write in
        full; it starts as the unwritten pattern. Anything else starts as sentinel bytes (fill it)."""
        if align < 1 or align & (align - 1):
            raise ValueError("align must be a power of two")
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        item = torch.empty(0, dtype=dtype).element_size()
        if align % item and item % align:
            raise ValueError("align must suit the element size")
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        ci, start = self._place(nbytes, max(align, item))
        c = self.chunks[ci]
        raw = c.buf[start:start + nbytes]
        if c.band is not None:
            c.band[start:start + nbytes] = False
        if written:
            raw.fill_(UNWRITTEN)
        view = raw.view(dtype).view(shape)
        a = max(align, item)
        assert view.data_ptr() % a == 0 and view.data_ptr() % (2 * a) != 0, name
        self.allocs.append(_Alloc(name, ci, start, nbytes, view, written))
        return view

    def put(self, src, align: int = 16, name: str = "?", frozen: bool = True) -> torch.Tensor:
        """A copy of `src` (tensor or array) in the arena; `frozen`: registered as an input."""
        src = torch.as_tensor(np.ascontiguousarray(src)) if not isinstance(src, torch.Tensor) else src.contiguous()
        t = self.alloc(tuple(src.shape), src.dtype, align, name)
        t.copy_(src)
        return self.freeze(t) if frozen else t

    def _find(self, t: torch.Tensor) -> _Alloc:
        for a in self.allocs:
            if a.view.data_ptr() == t.data_ptr() and a.view.numel() * a.view.element_size() == t.numel() * t.element_size():
                return a
        raise KeyError("not a tensor of this arena")

    def freeze(self, t: torch.Tensor) -> torch.Tensor:
        """Register `t` (an arena tensor, already filled) as an input: check() compares it with a clone."""
        self._find(t).frozen = t.clone()
        return t

    def thaw(self, t: torch.Tensor) -> torch.Tensor:
        self._find(t).frozen = None
        return t

    def rearm(self, t: torch.Tensor) -> torch.Tensor:
        """Refill a `written` output with the unwritten pattern before the next call that writes it."""
        a = self._find(t)
        self.chunks[a.chunk].buf[a.start:a.start + a.nbytes].fill_(UNWRITTEN)
        return t

    def backing(self, t: torch.Tensor):
        """(the uint8 backing buffer, the payload's first byte in it, its byte count) — for the self-test,
        which damages bands through the arena's own buffer."""
        a = self._find(t)
        return self.chunks[a.chunk].buf, a.start, a.nbytes

    # ------------------------------------------------------------------------------ the checks
    def _band_damage(self) -> Optional[str]:
        for ci, c in enumerate(self.chunks):
            mine = sorted((a for a in self.allocs if a.chunk == ci), key=lambda a: a.start)
            idx = c.damaged(mine)
            if idx is None:
                continue
            first, last, count = int(idx[0]), int(idx[-1]), int(idx.numel())
            msgs = []
            for k, a in enumerate(mine):     # attribute each damaged byte to the nearer payload
                lo = 0 if k == 0 else (mine[k - 1].start + mine[k - 1].nbytes + a.start) // 2
                end = a.start + a.nbytes
                hi = c.buf.numel() if k == len(mine) - 1 else (end + mine[k + 1].start) // 2
                before = idx[(idx >= lo) & (idx < a.start)]
                after = idx[(idx >= end) & (idx < hi)]
                if before.numel():
                    msgs.append(f"{before.numel()} byte(s) BEFORE '{a.name}', from {a.start - int(before[0])} B before its "
                                f"start")
                if after.numel():
                    msgs.append(f"{after.numel()} byte(s) PAST '{a.name}', up to {int(after[-1]) - end + 1} B past its end "
                                f"({a.nbytes} B payload)")
            return (f"guard band damaged ({count} byte(s), backing offsets {first}..{last}): " + "; ".join(msgs))
        return None

    def check(self, what: str = "") -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        tag = f"[{what}] " if what else ""
        msg = self._band_damage()
        assert msg is None, tag + msg
        for a in self.allocs:
            if a.written:
                raw = self.chunks[a.chunk].buf[a.start:a.start + a.nbytes]
                if a.nbytes % 4 == 0:
                    left = raw.view(torch.int32) == UNWRITTEN_I32
                else:
                    left = raw == UNWRITTEN
                n = int(left.sum())
                assert n == 0, (f"{tag}output '{a.name}': {n} element(s) left unwritten, the first at flat index "
                                f"{int(torch.nonzero(left.reshape(-1))[0])} of {left.numel()}")
            if a.frozen is not None:
                raw = a.view.reshape(-1).view(torch.uint8)
                ref = a.frozen.reshape(-1).view(torch.uint8)
                diff = raw != ref
                n = int(diff.sum())
                assert n == 0, (f"{tag}input '{a.name}' was modified: {n} byte(s), the first at byte "
                                f"{int(torch.nonzero(diff)[0])}")
