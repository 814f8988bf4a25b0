"""CPU: the host side of evaluate() (spwgnn_eval_metrics, added within ABI 8) — the export and its
signature against the header, every SPWGNN_E_ARG the header lists (fake pointers that are never followed, the
pattern of tests/test_loss_weights_host.py), spwgnn_amd.metrics against brute force on the quantised logits, the
numpy restatement tests/eval_ref.py against a hand-counted case, and Trainer.evaluate under gloo at world 2 (an
oracle engine whose eval_metrics is eval_ref) against the single-process dict."""
import ctypes as C
import math
import os
import re
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import eval_ref as ER
from oracle import model as O
from spwgnn_amd import _lib, data as D, engine as E, metrics as M, params as P
from spwgnn_amd.batch import TowerBatch
from spwgnn_amd.trainer import Trainer
from test_distributed import OracleEngine, _free_port

ROOT = Path(__file__).resolve().parents[1]
FAKE = 0x1000          # 8-byte aligned, never followed


# ---------------------------------------------------------------- the C ABI
def test_export_signature_and_struct_size():
    lib = _lib.lib()
    assert hasattr(lib, "spwgnn_eval_metrics")
    header = (ROOT / "include" / "spwgnn.h").read_text()
    proto = re.search(r"int32_t\s+spwgnn_eval_metrics\s*\((.*?)\)\s*;", header, re.S).group(1)
    n_args = len(re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(","))
    assert n_args == len(lib.spwgnn_eval_metrics.argtypes) == 5
    assert lib.spwgnn_eval_metrics.argtypes[3] == C.POINTER(_lib.EvalC)
    assert lib.spwgnn_struct_size(10) == C.sizeof(_lib.EvalC) == 16 + 6 * 8
    assert lib.spwgnn_struct_size(5) == -1 and lib.spwgnn_struct_size(8) == -1 and lib.spwgnn_struct_size(11) == -1
    assert lib.spwgnn_version() == 8 == _lib.ABI_VERSION                    # new symbols only: the ABI number stays
    assert f"#define SPWGNN_EVAL_BINS {_lib.EVAL_BINS}" in header and _lib.EVAL_BINS == M.BINS == ER.BINS == 256
    assert f"#define SPWGNN_EVAL_SIZES {_lib.EVAL_SIZES}" in header and _lib.EVAL_SIZES == M.SIZES == ER.SIZES == 33


def _ev(**kw):
    """A well-formed spwgnn_eval with every table and towers; `kw` overrides fields."""
    ev = _lib.EvalC()
    ev.rows, ev.n_towers, ev.threshold, ev.reserved = 5, 3, 0.5, 0
    ev.w = ev.tower_offsets = ev.node4 = ev.tower6 = ev.by_size = ev.hist = FAKE
    for k, v in kw.items():
        setattr(ev, k, v)
    return ev


def test_every_bad_argument_is_refused_before_any_device_work():
    lib = _lib.lib()

    def call(ev, logits=FAKE, targets=FAKE, n=12):
        return lib.spwgnn_eval_metrics(logits, targets, n, C.byref(ev) if ev is not None else None, None)

    bad = [
        call(_ev(), logits=None), call(_ev(), targets=None), call(None), call(_ev(node4=None)),      # null pointers
        call(_ev(), n=0), call(_ev(), n=-5),                                                          # n < 1
        call(_ev(rows=0)), call(_ev(rows=65)), call(_ev(rows=-1)),                                    # rows outside 1..64
        call(_ev(threshold=float("nan"))), call(_ev(threshold=0.0)), call(_ev(threshold=1.0)),        # tau outside (0, 1)
        call(_ev(threshold=-0.5)), call(_ev(threshold=1.5)), call(_ev(threshold=float("inf"))),
        call(_ev(reserved=1)),
        call(_ev(n_towers=-1)),
        call(_ev(tower_offsets=None)),                                                                # towers without offsets
        call(_ev(tower6=None, by_size=None)),                                                         # ... or without a tower table
        call(_ev(n_towers=0)),                                                                        # no towers, all three set
        call(_ev(n_towers=0, tower6=None, by_size=None)),                                             # ... offsets alone
        call(_ev(n_towers=0, tower_offsets=None, by_size=None)),                                      # ... tower6 alone
        call(_ev(n_towers=0, tower_offsets=None, tower6=None)),                                       # ... by_size alone
        call(_ev(node4=FAKE + 4)), call(_ev(tower6=FAKE + 4)), call(_ev(by_size=FAKE + 2)),           # misaligned tables
        call(_ev(hist=FAKE + 1)),
    ]
    assert bad == [_lib.E_ARG] * len(bad)


# ---------------------------------------------------------------- eval_ref itself, by hand
def test_eval_ref_on_a_hand_counted_case():
    #        tower 0 (3 nodes)        tower 1 (1)   tower 2 (2, masked)   tower 3 (2)
    z = [3.0, -2.0, 0.0,              -1.0,          9.0, 9.0,             2.0, float("nan")]
    t = [1.0, 0.0, 1.0,               1.0,           0.0, 0.0,             1.0, 1.0]
    w = [1.0, 2.0, 1.0,               0.5,           0.0, 0.0,             1.0, 1.0]
    off = [0, 3, 4, 6, 8]
    out = ER.eval_ref(z, t, w, off, 0.5)
    # TP: z=3 (t 1), z=2 (t 1); TN: z=-2 (t 0); FP: none; FN: z=0 (p = 0.5 is not > 0.5), z=-1, NaN
    assert out["node4"].tolist() == [[2, 1, 0, 3]]
    # towers counted: 0, 1, 3; none exact (tower 0 misses z = 0); actual-stable towers 1 and 3, no tower predicted stable
    assert out["tower6"].tolist() == [[3, 0, 0, 1, 0, 2]]
    assert out["by_size"][0, 3].tolist() == [1, 1, 0, 1, 1, 0] and out["by_size"][0, 1].tolist() == [0, 0, 0, 1, 1, 0]
    assert out["by_size"][0, 2].tolist() == [1, 0, 0, 1, 1, 0] and out["by_size"].sum() == 6 + 3
    h = out["hist"][0]
    assert h.sum() == 6 and h[0, (16 - 2) * 8] == 1 and h[1, (16 + 3) * 8] == 1 and h[1, 128] == 1 and h[1, 0] == 1
    # the bin is taken of the fp32 sum z + 16: the float just below 0.125 rounds up to the edge 16.125 (bin 129), the
    # float just below -15.875 keeps its distance in the sum (exact there) and falls into bin 0
    below = lambda e: np.nextafter(np.float32(e), np.float32(-100))
    assert ER.bins([-np.inf, -16.0, -15.9, 15.9375, 15.94, 16.0, np.inf, np.nan, 0.125, below(0.125), -15.875, below(-15.875)]
                   ).tolist() == [0, 0, 0, 255, 255, 255, 255, 0, 129, 129, 1, 0]
    # a target that is neither 0 nor 1 is a wrong prediction on the predicted side
    assert ER.eval_ref([4.0, -4.0], [0.5, 0.5])["node4"].tolist() == [[0, 0, 1, 1]]


# ---------------------------------------------------------------- metrics against brute force
def _random_hist(rng, n=400):
    z = rng.normal(scale=3.0, size=n).astype(np.float32)
    z[np.abs(z) < 0.125] = 1.0                       # nothing strictly inside the bins next to logit 0 ...
    z[:7] = 0.0                                      # ... except exact 0
    t = (rng.random(n) < 1 / (1 + np.exp(-z))).astype(np.float32)
    return z, t, ER.eval_ref(z, t)


def test_summarize_against_brute_force():
    rng = np.random.default_rng(5)
    z, t, tab = _random_hist(rng)
    h = tab["hist"][0]
    # the O(P·N) pair count on the quantised logits
    q = ER.bins(z)
    pos, neg = q[t == 1], q[t == 0]
    pairs = sum((p > neg).sum() + 0.5 * (p == neg).sum() for p in pos)
    auc = pairs / (len(pos) * len(neg))
    assert abs(M.roc_auc(h) - auc) <= 1e-12
    s = M.summarize(tab)
    assert abs(s["roc_auc"] - auc) <= 1e-12 and 0.5 < auc < 1.0
    tp, tn, fp, fn = (int(x) for x in tab["node4"][0])
    assert (s["tp"], s["tn"], s["fp"], s["fn"], s["n"]) == (tp, tn, fp, fn, len(z))
    assert s["binary_accuracy"] == (tp + tn) / len(z) and s["precision"] == tp / (tp + fp) and s["recall"] == tp / (tp + fn)
    assert s["specificity"] == tn / (tn + fp) and s["f1"] == 2 * tp / (2 * tp + fp + fn)
    # confusion_at on the histogram = a direct count at 0.5 (exact 0 is present and predicted "not stable")
    pred = ER.probability(z) > np.float32(0.5)
    direct = {"tp": int((pred & (t == 1)).sum()), "tn": int((~pred & (t == 0)).sum()),
              "fp": int((pred & (t == 0)).sum()), "fn": int((~pred & (t == 1)).sum())}
    assert M.confusion_at(h, 0.5) == direct == {"tp": tp, "tn": tn, "fp": fp, "fn": fn}
    # the ROC curve runs from (0, 0) to (1, 1), is monotone, and its trapezoid area is the rank AUC
    fpr, tpr, thr = M.roc_curve(h)
    assert (fpr[0], tpr[0], fpr[-1], tpr[-1]) == (0.0, 0.0, 1.0, 1.0) and len(thr) == 257
    assert np.all(np.diff(fpr) >= 0) and np.all(np.diff(tpr) >= 0) and np.all(np.diff(thr) <= 0)
    assert abs(float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2)) - auc) <= 1e-12
    for k in (100, 128, 140):     # a threshold on a bin edge: the curve's point is confusion_at's
        c = M.confusion_at(h, float(M.EDGE_PROBS[k]))
        j = 255 - k
        assert c["tp"] == round(tpr[j] * len(pos)) and c["fp"] == round(fpr[j] * len(neg))
    # best_threshold: no bin-edge threshold has a higher accuracy
    best = M.best_threshold(h)
    acc = lambda tau: (lambda c: c["tp"] + c["tn"])(M.confusion_at(h, tau))
    assert acc(best) == max(acc(float(p)) for p in M.EDGE_PROBS[1:-1]) >= tp + tn
    # average precision, the step definition, by brute force over the distinct quantised scores
    ap, prev = 0.0, 0.0
    for b in sorted(set(q.tolist()), reverse=True):
        sel = q >= b
        rec, prec = (sel & (t == 1)).sum() / len(pos), (sel & (t == 1)).sum() / sel.sum()
        ap, prev = ap + (rec - prev) * prec, rec
    assert abs(s["average_precision"] - ap) <= 1e-12


def test_summarize_tower_parts_rows_and_empty_classes():
    rng = np.random.default_rng(6)
    n, R = 60, 3
    z = rng.normal(scale=2.0, size=(R, n)).astype(np.float32)
    z[np.abs(z) < 0.01] = 1.0
    t = rng.integers(0, 2, n).astype(np.float32)
    off = np.concatenate([[0], np.cumsum([6] * 5 + [3] * 10)])
    tab = ER.eval_ref(z, t, None, off, 0.5)
    last, first = M.summarize(tab), M.summarize(tab, row=0)
    assert last == M.summarize(tab, row=R - 1) and first["tp"] == int(tab["node4"][0, 0])
    assert last["towers"] == 15 and set(last["by_size"]) == {3, 6}
    assert last["by_size"][6]["towers"] == 5 and last["by_size"][3]["n"] == 30
    t6 = tab["tower6"][-1]
    assert last["tower_exact_accuracy"] == t6[1] / 15 and last["tower_accuracy"] == (t6[2] + t6[3]) / 15
    assert (last["tower_tp"], last["tower_tn"], last["tower_fp"], last["tower_fn"]) == tuple(int(x) for x in t6[2:])
    assert sum(v["tp"] + v["tn"] + v["fp"] + v["fn"] for v in last["by_size"].values()) == last["n"]
    # node tables only: the tower and histogram keys are absent
    assert "towers" not in M.summarize({"node4": tab["node4"]}) and "roc_auc" not in M.summarize({"node4": tab["node4"]})
    # empty classes and empty tables: NaN, never a ZeroDivisionError
    only_pos = ER.eval_ref([1.0, 2.0], [1.0, 1.0])
    s = M.summarize(only_pos)
    assert math.isnan(s["roc_auc"]) and math.isnan(s["specificity"]) and s["recall"] == 1.0 and s["average_precision"] == 1.0
    only_neg = M.summarize(ER.eval_ref([1.0, -2.0], [0.0, 0.0]))
    assert math.isnan(only_neg["roc_auc"]) and math.isnan(only_neg["recall"]) and math.isnan(only_neg["average_precision"])
    empty = M.summarize({"node4": np.zeros((1, 4), np.int64), "tower6": np.zeros((1, 6), np.int64),
                         "by_size": np.zeros((1, 33, 6), np.int64), "hist": np.zeros((1, 2, 256), np.int64)})
    assert empty["n"] == 0 and empty["by_size"] == {} and all(
        math.isnan(empty[k]) for k in ("binary_accuracy", "precision", "recall", "f1", "tower_exact_accuracy", "roc_auc",
                                       "average_precision", "best_threshold"))
    for bad in (0.0, 1.0, float("nan")):
        try:
            M.confusion_at(tab["hist"][0], bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_eval_tables_on_the_host():
    a, b = E.EvalTables("cpu", rows=2), E.EvalTables("cpu", rows=2)
    assert a.flat.numel() == 2 * (4 + 6 + 33 * 6 + 512) and a.flat.dtype == torch.int64
    assert all(t.data_ptr() % 8 == 0 for t in a.tables.values())
    a.node4[1, 2] = 5
    b.hist[0, 1, 7] = 3
    b.by_size[1, 32, 5] = 2
    a.add_(b).add_(b)
    c = a.cpu()
    assert {k: v.shape for k, v in c.items()} == {"node4": (2, 4), "tower6": (2, 6), "by_size": (2, 33, 6), "hist": (2, 2, 256)}
    assert c["node4"][1, 2] == 5 and c["hist"][0, 1, 7] == 6 and c["by_size"][1, 32, 5] == 4 and a.flat.sum() == 15
    assert a.zero_().flat.sum() == 0
    small = E.EvalTables("cpu", towers=False, hist=False)
    assert set(small.cpu()) == {"node4"} and small.tower6 is None and small.hist is None
    for bad in (lambda: E.EvalTables("cpu", rows=0), lambda: E.EvalTables("cpu", rows=65), lambda: a.add_(small),
                lambda: E.check_threshold(float("nan")), lambda: E.check_threshold(1.0)):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("accepted")
    # the HIP path has no CPU fallback
    try:
        E.eval_metrics(torch.zeros(4), torch.zeros(4), small)
    except _lib.SpwgnnError:
        pass
    else:
        raise AssertionError("eval_metrics ran on CPU tensors")


# ---------------------------------------------------------------- Trainer.evaluate under gloo
class EvalOracleEngine(OracleEngine):
    """The oracle engine plus `eval_metrics` = eval_ref, and a correct count in its out3 (tests only)."""

    def loss(self, logits, target):   # out3 in fp64: the ranks' sums are compared to 1e-12
        loss, g = O.keras_bce_grad(logits.numpy(), target.numpy())
        return torch.tensor([loss, 0.0, float(logits.numel())], dtype=torch.float64), torch.tensor(g)

    def eval_metrics(self, logits, target, tables, batch, weights=None, threshold=0.5):
        off = np.concatenate([[0], np.cumsum(batch.tower_nodes)])
        ref = ER.eval_ref(logits.numpy(), target.numpy(), None if weights is None else np.asarray(weights), off, threshold)
        for k, t in tables.tables.items():
            t += torch.from_numpy(ref[k])
        return tables


EVAL_CUTS = [(0, 5), (5, 8)]   # world 2: 5 + 3 towers


def _eval_problem():
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(8, 5, seed=9, fully_connected=False)
    return obj, Rs, Rr, tgt


def _eval_trainer():
    params = P.to_flat(O.random_params(11), dtype=torch.float64)
    return Trainer(params, engine=EvalOracleEngine(), mp_steps=2, dropout=0.0)


def _eval_single():
    obj, Rs, Rr, tgt = _eval_problem()
    tr = _eval_trainer()
    before = tr.params.clone()
    out = tr.evaluate(TowerBatch.from_dense(obj, Rs, Rr, device="cpu"), torch.tensor(tgt.reshape(-1), dtype=torch.float64),
                      threshold=0.4)
    assert torch.equal(tr.params, before) and tr.iterations == 0        # no step was taken
    return out


def _eval_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    obj, Rs, Rr, tgt = _eval_problem()
    a, b = EVAL_CUTS[rank]
    if rank == 0:      # rank 0's shard as two micro-batches
        cuts = [(a, a + 2), (a + 2, b)]
    else:
        cuts = [(a, b)]
    batches = [TowerBatch.from_dense(obj[i:j], Rs[i:j], Rr[i:j], device="cpu") for i, j in cuts]
    targets = [torch.tensor(tgt[i:j].reshape(-1), dtype=torch.float64) for i, j in cuts]
    res = _eval_trainer().evaluate(batches, targets, threshold=0.4)
    torch.save(res, f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def _same(a, b) -> bool:
    """Equal dicts of ints, floats and such dicts: integer entries equal, and the ratios of equal integers with
    them (NaN equals NaN)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return type(a) is type(b) and a == b


def test_trainer_evaluate_gloo_world2_equals_single_process(tmp_path):
    out = str(tmp_path / "eval")
    mp.start_processes(_eval_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    ref = _eval_single()
    assert ref["n"] == 40 and ref["towers"] == 8 and set(ref["by_size"]) == {5}
    for rank in range(2):
        got = torch.load(f"{out}.{rank}", weights_only=False)
        assert abs(got["loss"] - ref["loss"]) <= 1e-12 * abs(ref["loss"]), (got["loss"], ref["loss"])
        assert _same({k: v for k, v in got.items() if k != "loss"}, {k: v for k, v in ref.items() if k != "loss"})
    # the evaluation run is fit's loss: the oracle's mean BCE over all 40 nodes
    obj, Rs, Rr, tgt = _eval_problem()
    tr = _eval_trainer()
    z = tr.engine.forward(tr.params, TowerBatch.from_dense(obj, Rs, Rr, device="cpu"), E.RunConfig(2))
    loss, _ = O.keras_bce_grad(z.numpy(), tgt.reshape(-1).astype(np.float64))
    assert abs(ref["loss"] - loss) <= 1e-12 * abs(loss)
