"""CPU: the guard-band helper (tests/guard.py) proves itself on CPU tensors. Every damaging write goes
through the arena's own backing buffer (`Arena.backing`), never outside an allocation."""
import pytest
import torch

import guard as G


def _arena():
    """An arena holding an output, an input and a 256-aligned scratch, as a guarded call would."""
    ar = G.Arena("cpu")
    out = ar.alloc((7, 100), torch.float32, name="out", written=True)
    inp = ar.put(torch.arange(33, dtype=torch.float32), name="inp")
    ws = ar.alloc(1000, torch.uint8, align=256, name="ws")
    return ar, out, inp, ws


def test_a_clean_run_passes():
    ar, out, inp, ws = _arena()
    out.copy_(torch.randn(7, 100))
    ws.fill_(0xFF)                       # scratch may hold anything
    ar.check("clean")
    ar.rearm(out)
    out.copy_(torch.zeros(7, 100))       # zeros are written values, not the unwritten pattern
    ar.check("clean again")


def test_layout_and_alignment():
    ar, out, inp, ws = _arena()
    for t, al in ((out, 16), (inp, 16), (ws, 256)):
        assert t.data_ptr() % al == 0 and t.data_ptr() % (2 * al) != 0      # the alignment asked for and no more
        buf, start, nbytes = ar.backing(t)
        assert nbytes == t.numel() * t.element_size()
        assert start >= G.BAND and start + nbytes + G.BAND <= buf.numel()
        assert bool((buf[start - G.BAND:start] == G.SENTINEL).all())
        assert bool((buf[start + nbytes:start + nbytes + G.BAND] == G.SENTINEL).all())
    assert out.is_contiguous() and out.shape == (7, 100)
    assert bool((out.reshape(-1).view(torch.int32) == G.UNWRITTEN_I32).all())
    assert torch.isfinite(out).all()                                          # the unwritten pattern is a finite float
    assert G.BAND > 128 * 100 * 4                                             # a 128-row tile of 100-float rows fits a band
    # payloads of one backing buffer are at least a band apart
    (_, s0, n0), (_, s1, _) = ar.backing(out), ar.backing(inp)
    assert s1 - (s0 + n0) >= G.BAND


def test_one_byte_past_the_end_is_detected():
    ar, out, inp, ws = _arena()
    out.fill_(1.0)
    buf, start, nbytes = ar.backing(out)
    buf[start + nbytes] = 0
    with pytest.raises(AssertionError, match=r"\[call 7\].*PAST 'out', up to 1 B past its end"):
        ar.check("call 7")
    buf[start + nbytes] = G.SENTINEL
    ar.check()
    buf2, s2, n2 = ar.backing(ws)       # the far end of a band, next to nothing else
    buf2[s2 + n2 + G.BAND - 1] = 1
    with pytest.raises(AssertionError, match=rf"PAST 'ws', up to {G.BAND} B past its end"):
        ar.check()


def test_one_byte_before_the_start_is_detected():
    ar, out, inp, ws = _arena()
    out.fill_(1.0)
    buf, start, _ = ar.backing(inp)
    buf[start - 1] = 0
    with pytest.raises(AssertionError, match=r"BEFORE 'inp', from 1 B before its start"):
        ar.check()
    buf[start - 1] = G.SENTINEL
    buf0, s0, _ = ar.backing(out)        # the first payload's leading band
    buf0[s0 - G.BAND] = 0
    with pytest.raises(AssertionError, match=rf"BEFORE 'out', from {G.BAND} B before its start"):
        ar.check()


def test_one_unwritten_element_is_detected():
    ar, out, inp, ws = _arena()
    with pytest.raises(AssertionError, match=r"output 'out': 700 element\(s\) left unwritten"):
        ar.check()
    out.fill_(0.5)
    ar.check()
    ar.rearm(out)
    vals = torch.randn(7, 100)
    out.copy_(vals)
    buf, start, _ = ar.backing(out)
    buf[start + 4 * 123:start + 4 * 124] = G.UNWRITTEN        # element 123 keeps the pattern
    with pytest.raises(AssertionError, match=r"output 'out': 1 element\(s\) left unwritten, the first at flat index 123"):
        ar.check()
    # an output whose size is no multiple of 4 is compared bytewise
    ar2 = G.Arena("cpu")
    o8 = ar2.alloc(7, torch.uint8, name="o8", written=True)
    o8[:6] = 1
    with pytest.raises(AssertionError, match=r"output 'o8': 1 element"):
        ar2.check()


def test_one_flipped_input_element_is_detected():
    ar, out, inp, ws = _arena()
    out.fill_(1.0)
    ar.check()
    buf, start, _ = ar.backing(inp)
    buf[start + 4 * 5] ^= 1                                     # the lowest mantissa bit of element 5
    with pytest.raises(AssertionError, match=r"input 'inp' was modified: 1 byte\(s\), the first at byte 20"):
        ar.check()
    buf[start + 4 * 5] ^= 1
    ar.check()
    inp[3] = float("nan")                                       # NaN != NaN: bits are compared, not values
    with pytest.raises(AssertionError, match="input 'inp' was modified"):
        ar.check()
    ar.freeze(inp)                                              # the NaN is now the registered content
    ar.check()


def test_large_requests_get_a_buffer_of_their_own():
    ar = G.Arena("cpu")
    a = ar.alloc(10, torch.float32, name="a", written=True)
    big = ar.alloc(G.CHUNK + 5, torch.uint8, align=256, name="big")
    b = ar.alloc(3, torch.float64, name="b", written=True)
    assert len(ar.chunks) >= 2
    a.zero_(), b.zero_()
    ar.check()
    buf, start, nbytes = ar.backing(big)
    buf[start + nbytes + 100] = 0
    with pytest.raises(AssertionError, match="PAST 'big', up to 101 B"):
        ar.check()
