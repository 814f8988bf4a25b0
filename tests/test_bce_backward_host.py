"""CPU: spwgnn_bce_backward refuses a loss size that is not the batch's node count (SPWGNN_E_ARG before any
device work; the folded loss indexes logits, targets and dlogits by plan node), and engine.bce_backward
raises before it reaches the library. Fake pointers that are never followed, as in
tests/test_loss_weights_host.py::test_statuses_without_a_device."""
import ctypes as C

import pytest
import torch

from spwgnn_amd import _lib, data as D, engine as E
from spwgnn_amd.batch import TowerBatch


def _structs():
    b = _lib.BatchC()
    b.n_towers, b.n_nodes, b.n_wtiles, b.n_eblocks, b.nw_max, b.flags = 2, 12, 2, 2, 6, 0
    fake = 0x1000
    b.pos = b.node_tower = b.node_local = b.wtile = b.edge_src = b.edge_dst = b.blk_csr = fake
    r = _lib.RunC()
    r.mp_steps, r.training, r.dropout, r.math = 3, 1, 0.0, _lib.MATH_X6
    return b, r, fake


def test_statuses_without_a_device():
    lib = _lib.lib()
    b, r, fake = _structs()
    need = lib.spwgnn_workspace_bytes(b.n_nodes, b.n_eblocks, r.mp_steps, 1)

    def bwd(n=b.n_nodes, nbytes=need, w3=None, t3=None, dprop=None):
        return lib.spwgnn_bce_backward(fake, C.byref(b), C.byref(r), fake, nbytes, fake, fake, n, fake, fake, fake,
                                       w3, t3, fake, dprop, None)

    for n in (b.n_nodes - 1, b.n_nodes + 1, 0, -1, 1 << 40):
        assert bwd(n=n) == _lib.E_ARG, n
        assert bwd(n=n, nbytes=need - 1) == _lib.E_ARG, n        # before the workspace is looked at
        assert bwd(n=n, dprop=fake, w3=fake, t3=fake) == _lib.E_ARG, n
    for math in (_lib.MATH_F32, _lib.MATH_X6, _lib.MATH_BF16, _lib.MATH_X3, _lib.MATH_H3):
        r.math = math
        assert bwd(n=b.n_nodes + 1) == _lib.E_ARG
        # the size check is the only thing in the way: the same well-formed call gets as far as the
        # workspace size (still before any device work)
        assert bwd(nbytes=need - 1) == _lib.E_WORKSPACE
    r.math = _lib.MATH_X6
    assert bwd(w3=fake) == _lib.E_ARG and bwd(t3=fake) == _lib.E_ARG   # the older checks still answer
    r.training = 0
    assert bwd() == _lib.E_NOTRAIN


def test_engine_refuses_a_logits_buffer_of_another_size():
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(2, 6, seed=3, fully_connected=True)
    batch = TowerBatch.from_dense(obj, Rs, Rr, device="cpu")
    run = E.RunConfig(3, training=True)
    for n in (batch.n_nodes - 1, batch.n_nodes + 1):
        with pytest.raises(ValueError, match="one value per node"):
            E.bce_backward(torch.zeros(1), batch, run, E.Workspace("cpu"), torch.zeros(n), torch.zeros(n), None)
