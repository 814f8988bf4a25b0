"""CPU: the host side of per-step logits and deep supervision (spwgnn_forward_steps, spwgnn_backward_steps,
spwgnn_bce_steps) — exports and struct sizes, the argument statuses that come back before any
device work, the front ends' validation of step_loss_weights, the oracle helper tests/steps_ref.py against
the states one S-step run returns, and the data-parallel Trainer with step_loss_weights under gloo (the oracle
as its engine) against the single-process step. Reference: the per-step readout x[:, :, :1] of Networks.py:89-94."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import steps_ref as SR
import x3_emu as X
from oracle import model as O
from spwgnn_amd import _lib, engine as E
from spwgnn_amd.keras_api import KerasModel, PropagationNetwork
from spwgnn_amd.network import GraphNetwork
from spwgnn_amd.trainer import Trainer

F64 = torch.float64
NEW_SYMBOLS = ("spwgnn_forward_steps", "spwgnn_backward_steps", "spwgnn_bce_steps", "spwgnn_bce_steps_scratch_bytes")
# sizeof of every ABI struct before this feature (spwgnn_struct_size's `which`): they must not move
OLD_SIZES = {0: 88, 1: 64, 2: 12, 3: 24, 4: 24, 5: -1, 6: 112, 7: 32, 8: -1}


def test_exports_signatures_and_struct_sizes():
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    pb, pr = C.POINTER(_lib.BatchC), C.POINTER(_lib.RunC)
    # (params, batch, run, workspace, workspace_bytes, step_logits, state_out, stream)
    assert lib.spwgnn_forward_steps.argtypes == [vp, pb, pr, vp, i64, vp, vp, vp]
    # (params, batch, run, workspace, workspace_bytes, dstep_logits, dstate, grads, dprop, stream)
    assert lib.spwgnn_backward_steps.argtypes == [vp, pb, pr, vp, i64, vp, vp, vp, vp, vp]
    assert lib.spwgnn_bce_steps_scratch_bytes.argtypes == [i64, i32]
    assert lib.spwgnn_bce_steps.argtypes[:6] == [vp, vp, i64, i32, C.POINTER(_lib.StepWeightsC),
                                                 C.POINTER(_lib.LossWeightsC)]
    assert len(lib.spwgnn_bce_steps.argtypes) == 14
    assert lib.spwgnn_version() == 8 == _lib.ABI_VERSION                    # new symbols only: the ABI number stays
    for which, size in OLD_SIZES.items():
        assert lib.spwgnn_struct_size(which) == size, which
    for which, st in ((0, _lib.BatchC), (1, _lib.RunC), (2, _lib.PlanSizes), (3, _lib.ParamInfo),
                      (4, _lib.LossWeightsC), (6, _lib.PlanDeviceC), (7, _lib.ClipC)):
        assert C.sizeof(st) == OLD_SIZES[which]
    assert lib.spwgnn_struct_size(9) == C.sizeof(_lib.StepWeightsC) == 8 + 4 * 64
    assert lib.spwgnn_bce_steps_scratch_bytes(10, 5) == 5 * lib.spwgnn_bce_scratch_bytes(10)
    assert lib.spwgnn_bce_steps_scratch_bytes(10, 0) == -1 and lib.spwgnn_bce_steps_scratch_bytes(10, 65) == -1


def _sw(lam, count=None):
    sw = _lib.StepWeightsC()
    sw.count = len(lam) if count is None else count
    for s, x in enumerate(lam):
        sw.lam[s] = x
    return sw


def test_bce_steps_refusals_without_a_device():
    """Every refusal comes back before a launch: the pointers are never followed."""
    lib = _lib.lib()
    fake = 0x1000

    def call(lam, S=3, count=None, n=12, lw=None, w3=None, t3=None, t3s=None, logits=fake, out3s=fake, sw=True):
        return lib.spwgnn_bce_steps(logits, fake, n, S, C.byref(_sw(lam, count)) if sw else None,
                                    C.byref(lw) if lw is not None else None, out3s, fake, fake, fake, w3, t3, t3s, None)

    good = [0.2, 0.3, 0.5]
    assert call(good, sw=False) == _lib.E_ARG                       # no step weights
    assert call(good, logits=None) == _lib.E_ARG and call(good, out3s=None) == _lib.E_ARG
    assert call(good, n=0) == _lib.E_ARG
    assert call([0.5, 0.5], S=3) == _lib.E_ARG                      # a count other than mp_steps
    assert call(good, S=3, count=4) == _lib.E_ARG
    assert call(good, S=0, count=0) == _lib.E_ARG and call([1.0] * 64, S=65, count=65) == _lib.E_ARG
    assert call([0.2, -0.1, 0.9]) == _lib.E_ARG                     # negative
    assert call([0.2, float("nan"), 0.9]) == _lib.E_ARG             # non-finite
    assert call([0.2, float("inf"), 0.9]) == _lib.E_ARG
    assert call([0.0, 0.0, 0.0]) == _lib.E_ARG                      # all zero
    assert call([0.0, -0.0, 0.0]) == _lib.E_ARG
    assert call(good, w3=fake) == _lib.E_ARG and call(good, t3=fake) == _lib.E_ARG   # weights3 / total3 go together
    assert call(good, t3s=fake) == _lib.E_ARG                       # total3s needs them
    bad_lw = _lib.LossWeightsC()
    bad_lw.w, bad_lw.norm = fake, 0.0
    assert call(good, lw=bad_lw) == _lib.E_ARG                      # spwgnn_bce_weighted's rules
    no_w = _lib.LossWeightsC()
    no_w.norm = 12.0
    assert call(good, lw=no_w) == _lib.E_ARG


def test_forward_backward_steps_statuses_without_a_device():
    lib = _lib.lib()
    b = _lib.BatchC()
    b.n_towers, b.n_nodes, b.n_wtiles, b.n_eblocks, b.nw_max, b.flags = 2, 12, 2, 2, 6, 0
    fake = 0x1000
    b.pos = b.node_tower = b.node_local = b.wtile = b.edge_src = b.edge_dst = b.blk_csr = fake
    r = _lib.RunC()
    r.mp_steps, r.training, r.dropout, r.math = 3, 1, 0.0, _lib.MATH_X6
    need = lib.spwgnn_workspace_bytes(b.n_nodes, b.n_eblocks, r.mp_steps, 1)
    fwd = lambda z=fake, st=None, nb=need - 1: lib.spwgnn_forward_steps(fake, C.byref(b), C.byref(r), fake, nb, z, st, None)
    bwd = lambda dz=fake, ds=None, g=fake, nb=need - 1: lib.spwgnn_backward_steps(fake, C.byref(b), C.byref(r), fake, nb,
                                                                                    dz, ds, g, None, None)
    assert fwd(z=None) == _lib.E_ARG and fwd(st=0x1004) == _lib.E_ARG       # null rows; a misaligned state
    assert bwd(dz=None) == _lib.E_ARG and bwd(g=None) == _lib.E_ARG and bwd(ds=0x1004) == _lib.E_ARG
    assert fwd() == _lib.E_WORKSPACE and bwd() == _lib.E_WORKSPACE           # well formed: as far as the size check
    r.training = 0
    assert bwd() == _lib.E_NOTRAIN
    r.training, r.mp_steps = 1, 65
    assert fwd() == _lib.E_SHAPE


@pytest.mark.parametrize("bad", [[0.5, 0.5], [0.2] * 6, [0.2, 0.2, -0.1, 0.2, 0.5], [0.0] * 5,
                                 [0.2, 0.2, float("nan"), 0.2, 0.2]], ids=["short", "long", "negative", "zero", "nan"])
def test_front_ends_validate_step_loss_weights(bad):
    net = GraphNetwork(device="cpu")          # mp_steps = 5
    with pytest.raises(ValueError):
        KerasModel(net, 4, step_loss_weights=bad)
    with pytest.raises(ValueError):
        PropagationNetwork(device="cpu", step_loss_weights=bad)
    with pytest.raises(ValueError):
        E.check_step_weights(bad, 5)

    class NoSteps:   # an engine without the hook is refused before anything runs
        pass

    with pytest.raises(ValueError):
        Trainer(torch.zeros(8), engine=NoSteps(), step_loss_weights=bad)


def test_none_is_the_model_of_before():
    """step_loss_weights=None adds nothing: the update choice, the replay options and the buffers."""
    plain = PropagationNetwork(device="cpu").getModel(4)
    assert plain.step_loss_weights is None and plain._path.lam is None and plain._tot_s is None
    assert plain._clip_on() is False and plain._replay_graph is None and plain.history == {}
    deep = PropagationNetwork(device="cpu", step_loss_weights=[0.1, 0.1, 0.1, 0.2, 0.5]).getModel(4)
    assert deep.step_loss_weights == (0.1, 0.1, 0.1, 0.2, 0.5) and deep._clip_on() is False
    assert deep._tot_s.shape == (5, 3) and deep._tot_s.dtype == torch.float64
    # the replayed step's option tuple grows only with weights set (fit() compares it to rebuild its cache)
    src = inspect.getsource(KerasModel.fit)
    assert "if lam is not None:\n            opts += (lam,)" in src
    assert inspect.signature(KerasModel.predict).parameters["return_steps"].default is False
    for fn in (GraphNetwork.forward_batch, GraphNetwork.forward_logits, GraphNetwork.forward):
        assert inspect.signature(fn).parameters["return_steps"].default is False
    tr = Trainer(torch.zeros(8), engine=object())
    assert tr.step_loss_weights is None


# ------------------------------------------------------------------------- the oracle helper
@pytest.mark.parametrize("fully", [True, False], ids=["full", "thr"])
def test_step_logits_agree_with_the_states_of_one_run(fully):
    """z_s = forward_dense(mp_steps = s + 1) is the per-step readout: recomputed from states[s] of ONE S-step run
    through one more pass it is the same number (fp64: to rounding), and its last row is the run's own logits."""
    S = 4
    obj, Rs, Rr = X.dense_case(3, 5, fully)[:3]
    groups = [(obj, Rs, Rr)]
    n = obj.shape[0] * obj.shape[1]
    tp = O.to_torch(O.random_params(5))
    objs = [torch.tensor(obj, dtype=F64)]
    prop = torch.tensor(np.random.default_rng(3).normal(0, 0.3, (n, 100)), dtype=F64)
    with torch.no_grad():
        Z = SR.step_logits(tp, groups, objs, prop, S)
        Zs = SR.step_logits_from_states(tp, groups, objs, prop, S)
        z_last = O.forward_dense(tp, objs[0], torch.as_tensor(Rs, dtype=F64), torch.as_tensor(Rr, dtype=F64),
                                 prop.reshape(3, 5, 100), S).reshape(-1)
    assert Z.shape == (S, n)
    assert float((Z - Zs).abs().max()) <= 1e-12
    assert torch.equal(Z[-1], z_last)
    assert float((Z[0] - Z[-1]).abs().max()) > 1e-3          # the rows really differ


def test_deep_loss_and_numpy_loss_agree():
    rng = np.random.default_rng(0)
    S, n = 3, 17
    Z = rng.normal(scale=3.0, size=(S, n)).astype(np.float32)
    t = rng.integers(0, 2, n).astype(np.float64)
    lam = [0.25, 0.0, 0.75]
    w = rng.choice([0.0, 0.5, 2.0], size=n)
    for ww, norm in ((None, None), (w, float(max(np.count_nonzero(w), 1)))):
        Zt = torch.tensor(Z, dtype=F64, requires_grad=True)
        loss = SR.deep_loss(Zt, torch.tensor(t), lam, None if ww is None else torch.tensor(ww), norm)
        loss.backward()
        out3s, out3, dl = SR.bce_steps_numpy(Z, t, lam, ww, norm)
        assert abs(float(loss.detach()) - out3[0]) <= 1e-12
        assert np.abs(Zt.grad.numpy() - dl).max() <= 1e-15
        assert np.all(dl[1] == 0.0)


# ---------------------------------------------------------------- gloo data parallel
import os  # noqa: E402

import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

import test_loss_weights_host as LW  # noqa: E402
from spwgnn_amd import params as P  # noqa: E402
from spwgnn_amd.batch import TowerBatch  # noqa: E402

DP_S, DP_LAM = 3, (0.2, 0.0, 0.8)


class StepsOracleEngine(LW.WeightedOracleEngine):
    """The fp64 oracle behind the Trainer's engine interface with per-step rows (tests only): "logits" are the
    (S, n) rows z_s = the network at s + 1 steps, the loss is Σ_s λ_s·BCE(z_s)."""

    def set_step_loss_weights(self, lam, mp_steps):
        assert len(lam) == mp_steps
        self.lam = tuple(lam)

    def forward(self, flat, batch, run):
        self.p = self._params(flat)
        pos = batch.pos[:, :3].to(torch.float64)
        src = torch.as_tensor(batch.src, dtype=torch.long)
        dst = torch.as_tensor(batch.dst, dtype=torch.long)
        prop = torch.zeros(batch.n_nodes, 100, dtype=torch.float64)
        self.z = torch.stack([O.forward_gather(self.p, pos, src, dst, prop, k + 1) for k in range(run.mp_steps)])
        return self.z.detach()

    def loss(self, logits, target):
        _, out3, dl = SR.bce_steps_numpy(logits.numpy(), target.numpy(), self.lam)
        return torch.tensor(out3), torch.tensor(dl)

    def loss_weighted(self, logits, target, weights, norm):
        _, out3, dl = SR.bce_steps_numpy(logits.numpy(), target.numpy(), self.lam, weights.numpy(), norm)
        return torch.tensor(out3), torch.tensor(dl)


def _dp_trainer():
    params = P.to_flat(O.random_params(11), dtype=torch.float64)
    tr = Trainer(params, engine=StepsOracleEngine(), mp_steps=DP_S, dropout=0.0, step_loss_weights=DP_LAM)
    tr.m, tr.v = torch.zeros_like(params), torch.zeros_like(params)
    return params, tr


def _dp_run(tr, batch, tgt, W, weighted):
    t = torch.tensor(tgt.reshape(-1), dtype=torch.float64)
    return tr.step(batch, t, weights=torch.tensor(W.reshape(-1))) if weighted else tr.step(batch, t)


def _dp_single(steps, weighted):
    obj, Rs, Rr, tgt, W = LW._dp_problem()
    params, tr = _dp_trainer()
    for _ in range(steps):
        out3 = _dp_run(tr, TowerBatch.from_dense(obj, Rs, Rr, device="cpu"), tgt, W, weighted)
    return params.numpy(), out3


def _dp_worker(rank, world, port, steps, weighted, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    obj, Rs, Rr, tgt, W = LW._dp_problem()
    sh = slice(*LW.DP_CUTS[rank])
    params, tr = _dp_trainer()
    for _ in range(steps):
        _dp_run(tr, TowerBatch.from_dense(obj[sh], Rs[sh], Rr[sh], device="cpu"), tgt[sh], W[sh], weighted)
    if rank == 0:
        np.save(out, params.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "node_weights"])
def test_dp_gloo_world2_deep_supervision_equals_full_batch(tmp_path, weighted):
    """World 2 (4 + 3 towers of 5 boxes), S = 3, λ = (0.2, 0, 0.8): the Trainer hands the (S, n) rows through its
    scaling and its all-reduce untouched — the parameters after 2 steps equal the single-process step on the full
    batch to tests/test_distributed.py's 1e-9 — and the single-process result is the oracle's deep loss."""
    out = str(tmp_path / "p.npy")
    mp.start_processes(_dp_worker, args=(2, LW._free_port(), 2, weighted, out), nprocs=2, join=True, start_method="spawn")
    ref, out3 = _dp_single(2, weighted)
    assert np.abs(np.load(out) - ref).max() < 1e-9
    start = P.to_flat(O.random_params(11), dtype=torch.float64).numpy()
    assert np.abs(ref - start).max() > 1e-6                                   # it moved
    # and not where the last-step loss alone would move it
    params = P.to_flat(O.random_params(11), dtype=torch.float64)
    tr = Trainer(params, engine=StepsOracleEngine(), mp_steps=DP_S, dropout=0.0, step_loss_weights=(0.0, 0.0, 1.0))
    tr.m, tr.v = torch.zeros_like(params), torch.zeros_like(params)
    obj, Rs, Rr, tgt, W = LW._dp_problem()
    for _ in range(2):
        _dp_run(tr, TowerBatch.from_dense(obj, Rs, Rr, device="cpu"), tgt, W, weighted)
    assert np.abs(params.numpy() - ref).max() > 1e-6
    assert float(out3[2]) == (np.count_nonzero(W) if weighted else tgt.size)
