"""CPU: the host side of the clipped Adam step (spwgnn_adam_clipped) — the ABI, the
argument checks (all return before any launch, so no GPU is needed), the decayed lr tables, the
Trainer's arguments, and the data-parallel control flow under gloo with the fp64 oracle engine.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import clip_ref as R
import test_distributed as TD
from oracle import model as O
from spwgnn_amd import _lib, params as P
from spwgnn_amd.batch import TowerBatch
from spwgnn_amd.trainer import Trainer


# ---------------------------------------------------------------- ABI
def test_exports_and_struct_size():
    L = _lib.lib()
    for name in ("spwgnn_clip_scratch_bytes", "spwgnn_adam_clipped", "spwgnn_adam_clipped_dev",
                 "spwgnn_adam_lr_decayed", "spwgnn_adam_lr_table_decay"):
        assert hasattr(L, name), name
    assert L.spwgnn_struct_size(7) == C.sizeof(_lib.ClipC) == 32
    assert L.spwgnn_struct_size(5) == -1 and L.spwgnn_struct_size(8) == -1
    assert L.spwgnn_clip_scratch_bytes() >= 4
    assert L.spwgnn_version() == 8


# ---------------------------------------------------------------- argument checks (no launch)
def _clip(clipnorm=1.0, clipvalue=0.0, out4=0x1000, total4=None):
    c = _lib.ClipC()
    c.clipnorm, c.clipvalue, c.skip_nonfinite, c.out4, c.total4 = clipnorm, clipvalue, 0, out4, total4
    return c


def _call(dev, clip, scratch=0x2000, n=None, ptrs=(0x3000, 0x4000, 0x5000, 0x6000), step=1, step_dev=0x7000,
          table=0x8000, table_len=16):
    """The entry point with fake (never dereferenced: every case here is rejected first) pointers."""
    L = _lib.lib()
    n = P.flat_size() if n is None else n
    cp = C.byref(clip) if clip is not None else None
    if dev:
        return L.spwgnn_adam_clipped_dev(*ptrs, n, step_dev, table, table_len, 0.9, 0.999, 1e-7, 0.0, 1.0, cp,
                                         scratch, None)
    return L.spwgnn_adam_clipped(*ptrs, n, step, 5e-4, 0.9, 0.999, 1e-7, 0.0, 1.0, cp, scratch, None)


@pytest.mark.parametrize("dev", [False, True])
def test_argument_errors_return_before_any_launch(dev):
    ok = (0x3000, 0x4000, 0x5000, 0x6000)
    for k in range(4):                                    # params, grads, m, v
        ptrs = tuple(None if i == k else p for i, p in enumerate(ok))
        assert _call(dev, _clip(), ptrs=ptrs) == _lib.E_ARG, k
    assert _call(dev, None) == _lib.E_ARG                 # no struct
    assert _call(dev, _clip(out4=None)) == _lib.E_ARG     # no out4
    assert _call(dev, _clip(), scratch=None) == _lib.E_ARG
    for n in (P.flat_size() - 64, P.flat_size() + 64, P.real_size(), 0, -1):
        assert _call(dev, _clip(), n=n) == _lib.E_ARG, n
    for bad in (-1.0, -1e-30, float("nan"), -float("inf")):
        assert _call(dev, _clip(clipnorm=bad)) == _lib.E_ARG, bad
        assert _call(dev, _clip(clipnorm=0.0, clipvalue=bad)) == _lib.E_ARG, bad
    if dev:
        assert _call(dev, _clip(), step_dev=None) == _lib.E_ARG
        assert _call(dev, _clip(), table=None) == _lib.E_ARG
        assert _call(dev, _clip(), table_len=1) == _lib.E_ARG
    else:
        assert _call(dev, _clip(), step=0) == _lib.E_ARG


# ---------------------------------------------------------------- lr tables
LR, B1, B2 = (float(np.float32(x)) for x in (5e-4, 0.9, 0.999))   # the fp32 values the library receives


def _table(n, decay=None, lr=LR):
    out = np.full(n, -1.0, np.float32)
    L = _lib.lib()
    st = (L.spwgnn_adam_lr_table(lr, B1, B2, n, out.ctypes.data) if decay is None else
          L.spwgnn_adam_lr_table_decay(lr, decay, B1, B2, n, out.ctypes.data))
    assert st == 0
    return out


def test_lr_table_decay_zero_is_the_plain_table_bitwise():
    a, b = _table(5000), _table(5000, 0.0)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    out = np.zeros(4, np.float32)
    L = _lib.lib()
    assert L.spwgnn_adam_lr_table_decay(LR, -1.0, B1, B2, 4, out.ctypes.data) == _lib.E_ARG
    assert L.spwgnn_adam_lr_table_decay(LR, float("nan"), B1, B2, 4, out.ctypes.data) == _lib.E_ARG
    assert L.spwgnn_adam_lr_table_decay(LR, 0.1, B1, B2, 1, out.ctypes.data) == _lib.E_ARG
    assert L.spwgnn_adam_lr_table_decay(LR, 0.1, B1, B2, 4, None) == _lib.E_ARG


def test_lr_table_decay_within_2ulp_of_fp64_formula():
    """lr_t = lr / (1 + d·(t − 1)) · sqrt(1 − β2^t) / (1 − β1^t) in fp64 on the fp32 arguments; the
    library rounds lr_eff to fp32 and then lr_t: two roundings, under 2 ulp."""
    n, d = 5000, float(np.float32(1e-3))
    got = _table(n, d)
    t = np.arange(1, n, dtype=np.float64)
    lr, b1, b2, dd = (np.float64(x) for x in (LR, B1, B2, d))
    ref = lr / (1.0 + dd * (t - 1.0)) * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    assert got[0] == 0.0
    ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got[1:].astype(np.float64) - ref) <= 2.0 * ulp)
    assert got[-1] < 0.25 * _table(n)[-1]                      # it decays


def test_eager_helper_and_table_agree_bitwise():
    """An eager step passes spwgnn_adam_lr_decayed(lr, d, t − 1) as its lr; the kernel's lr_t is then the
    plain table's entry t for that lr — the decayed table's entry t, bit for bit."""
    L = _lib.lib()
    d = float(np.float32(1e-3))
    tab = _table(1001, d)
    assert L.spwgnn_adam_lr_decayed(LR, d, 0) == float(LR)
    assert L.spwgnn_adam_lr_decayed(LR, 0.0, 77) == float(LR)
    for t in (1, 2, 1000):
        lr_eff = L.spwgnn_adam_lr_decayed(LR, d, t - 1)   # a c_float: already an fp32 value
        assert abs(float(lr_eff) - float(LR) / (1.0 + float(d) * (t - 1))) <= np.spacing(np.float32(lr_eff))
        assert _table(t + 1, None, lr_eff)[t].view(np.uint32) == tab[t].view(np.uint32), t


# ---------------------------------------------------------------- Trainer arguments
class _NoClipEngine:
    """An engine of before this feature: no adam_clipped."""

    def adam(self, *a):
        pass


class _AssertingEngine(TD.OracleEngine):
    def adam_clipped(self, *a):
        raise AssertionError("adam_clipped called with every option off")


def test_trainer_argument_checks():
    params = torch.zeros(P.flat_size(), dtype=torch.float64)
    for kw in (dict(clipnorm=-1), dict(clipvalue=-0.5), dict(decay=-1e-3), dict(clipnorm=float("nan"))):
        with pytest.raises(ValueError):
            Trainer(params, engine=TD.OracleEngine(), **kw)
    for kw in (dict(clipnorm=1.0), dict(clipvalue=1.0), dict(decay=0.1), dict(skip_nonfinite=True)):
        with pytest.raises(ValueError, match="adam_clipped"):
            Trainer(params, engine=_NoClipEngine(), **kw)
    Trainer(params, engine=_NoClipEngine())   # options off: such an engine is fine


def test_options_off_never_call_adam_clipped():
    obj, Rs, Rr, tgt = TD._problem()
    batch = TowerBatch.from_dense(obj, Rs, Rr, device="cpu")
    params = P.to_flat(O.random_params(11), dtype=torch.float64)
    tr = Trainer(params, engine=_AssertingEngine(), mp_steps=3, dropout=0.0)
    tr.m, tr.v = torch.zeros_like(params), torch.zeros_like(params)
    tr.step(batch, torch.tensor(tgt.reshape(-1), dtype=torch.float64))
    assert tr.clip_stats is None and tr.iterations == 1
    assert np.abs(params.numpy() - TD._single(1)).max() == 0.0   # today's step


# ---------------------------------------------------------------- gloo, world 2
class ClipOracleEngine(TD.OracleEngine):
    """The fp64 oracle engine with the restated clipped update (numpy, in place)."""

    def adam_clipped(self, params, grads, m, v, step, lr, b1, b2, eps, l2, gscale, clipnorm, clipvalue,
                     skip_nonfinite):
        p2, m2, v2, info = R.step(params.numpy(), grads.numpy(), m.numpy(), v.numpy(), step, lr, b1, b2, eps, l2,
                                  gscale, clipnorm, clipvalue, 0.0, skip_nonfinite, mask=R.real_mask())
        params.copy_(torch.from_numpy(p2))
        m.copy_(torch.from_numpy(m2))
        v.copy_(torch.from_numpy(v2))
        return torch.tensor([info["norm"], info["scale"], float(info["skipped"]), float(info["clipped"])],
                            dtype=torch.float64)


def _step1_norm():
    """The global gradient norm of the full-batch problem's first step (fp64 oracle)."""
    obj, Rs, Rr, tgt = TD._problem()
    batch = TowerBatch.from_dense(obj, Rs, Rr, device="cpu")
    params = P.to_flat(O.random_params(11), dtype=torch.float64)
    eng = TD.OracleEngine()
    t = torch.tensor(tgt.reshape(-1), dtype=torch.float64)
    _, dz = eng.loss(eng.forward(params, batch, type("R", (), {"mp_steps": 3})()), t)
    return R.global_norm(eng.backward(params, batch, None, dz).numpy(), R.real_mask())


def _clipped_single(steps, clipnorm):
    obj, Rs, Rr, tgt = TD._problem()
    batch = TowerBatch.from_dense(obj, Rs, Rr, device="cpu")
    params = P.to_flat(O.random_params(11), dtype=torch.float64)
    tr = Trainer(params, engine=ClipOracleEngine(), mp_steps=3, dropout=0.0, clipnorm=clipnorm)
    tr.m, tr.v = torch.zeros_like(params), torch.zeros_like(params)
    norms = []
    for _ in range(steps):
        tr.step(batch, torch.tensor(tgt.reshape(-1), dtype=torch.float64))
        norms.append(float(tr.clip_stats[0]))
        assert float(tr.clip_stats[3]) == float(norms[-1] >= clipnorm)
    assert norms[0] >= clipnorm                       # the first step clips (the norm then falls quickly)
    return params.numpy(), norms


def _clip_worker(rank, world, port, steps, out, clipnorm, overlap):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    obj, Rs, Rr, tgt = TD._problem()
    sh = slice(rank * 4, rank * 4 + 4)
    batch = TowerBatch.from_dense(obj[sh], Rs[sh], Rr[sh], device="cpu")
    params = P.to_flat(O.random_params(11), dtype=torch.float64)
    eng = ClipOracleEngine()
    if overlap:
        eng.early_event = lambda: "reached"
    tr = Trainer(params, engine=eng, mp_steps=3, dropout=0.0, clipnorm=clipnorm)
    assert tr._split() == overlap
    tr.m, tr.v = torch.zeros_like(params), torch.zeros_like(params)
    norms = []
    for _ in range(steps):
        tr.step(batch, torch.tensor(tgt[sh].reshape(-1), dtype=torch.float64))
        norms.append(float(tr.clip_stats[0]))
    np.save(f"{out}.{rank}.npy", np.concatenate([params.numpy(), np.array(norms)]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [False, True])
def test_dp_gloo_world2_clipped_equals_full_batch(tmp_path, overlap):
    """The norm is taken after the all-reduce (with `overlap`: after both pieces are back), so both ranks
    clip by the same norm — bitwise — and three clipped DP steps equal the single-process run to 1e-9,
    tests/test_distributed.py's bound for the same comparison."""
    c = 0.5 * _step1_norm()
    out = str(tmp_path / "p")
    mp.start_processes(_clip_worker, args=(2, TD._free_port(), 3, out, c, overlap), nprocs=2, join=True,
                       start_method="spawn")
    r0, r1 = np.load(out + ".0.npy"), np.load(out + ".1.npy")
    ref, norms = _clipped_single(3, c)
    assert np.array_equal(r0[-3:].view(np.uint64), r1[-3:].view(np.uint64))   # the ranks' norms, bit for bit
    assert np.array_equal(r0, r1)
    assert np.abs(r0[:-3] - ref).max() < 1e-9
    assert np.abs(r0[-3:] - np.array(norms)).max() <= 1e-9 * max(norms)
    assert np.abs(ref - TD._single(3)).max() > 1e-6          # the clip changed the trajectory
