"""GPU: spwgnn_bce_tower (the tower-level loss) against the fp64 restatement tests/tower_loss_ref.py,
its bit contracts with spwgnn_bce / spwgnn_bce_weighted, masks, agreement with spwgnn_eval_metrics' tower table,
and guard bands around every caller-owned buffer.

Shapes: towers of {1}, {32} and a ragged mix of 1..32 nodes; 1 tower, and 255 / 256 / 257 towers (one below, at
and one above what a workgroup's 256 threads take); the one-launch form (n <= 256 and n_towers <= 256) and the
two-launch form; 65,537 one-node towers, where the 256 tower workgroups take a second tower per thread.
Logits: per tower N(offset, sigma) with (sigma, offset) drawn from {0.5, 2, 4, 8} x {0, 3, 6, 10}, so both
tower labels see s_u from below the lower clip to above the upper one."""
import functools
import types

import numpy as np
import pytest
import torch

import guard as G
import tower_loss_ref as TR
from spwgnn_amd import _lib, engine as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
SIGMAS, OFFSETS = (0.5, 2.0, 4.0, 8.0), (0.0, 3.0, 6.0, 10.0)
# (name, tower sizes): one launch above the line, two below
SHAPES = {
    "one_1x1": [1], "one_1x32": [32], "one_255x1": [1] * 255, "one_256x1": [1] * 256, "one_8x32": [32] * 8,
    "one_ragged": "ragged:14:240",
    "two_257x1": [1] * 257, "two_9x32": [32] * 9, "two_255x32": [32] * 255, "two_256x32": [32] * 256,
    "two_257x32": [32] * 257, "two_ragged255": "ragged:255", "two_ragged256": "ragged:256",
    "two_ragged257": "ragged:257", "two_65537x1": [1] * 65537,
}


def _sizes(spec, rng):
    if not isinstance(spec, str):
        return np.asarray(spec, np.int64)
    parts = spec.split(":")
    T = int(parts[1])
    s = rng.integers(1, 33, T)
    s[:min(T, 32)] = rng.permutation(np.arange(1, 33))[:min(T, 32)]
    if len(parts) > 2:                                   # a node budget: shrink the largest until it fits
        while s.sum() > int(parts[2]):
            s[np.argmax(s)] -= 1
    return s


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(z, node targets, weights, offsets, explicit tower targets) as read-only numpy arrays, built once."""
    rng = np.random.default_rng(sorted(SHAPES).index(name) + 100)
    sizes = _sizes(SHAPES[name], rng)
    T, n = len(sizes), int(sizes.sum())
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    tower = np.repeat(np.arange(T), sizes)
    sg = rng.choice(SIGMAS, T)[tower]
    of = rng.choice(OFFSETS, T)[tower]
    z = (rng.normal(size=n) * sg + of).astype(np.float32)
    all_one = rng.random(T) < 0.5                        # derived labels of both kinds at every size
    t = np.where(all_one[tower], 1.0, (rng.random(n) < 0.7)).astype(np.float32)
    w = rng.choice(np.array([0.0, 0.5, 1.0, 2.5], np.float32), size=n, p=[0.3, 0.25, 0.25, 0.2])
    tt = rng.integers(0, 2, T).astype(np.float32)
    for a in (z, t, w, off, tt):
        a.setflags(write=False)
    return z, t, w, off, tt


def fake_batch(off):
    off = np.asarray(off)
    return types.SimpleNamespace(n_nodes=int(off[-1]), n_towers=len(off) - 1, tower_nodes=np.diff(off),
                                 tower_offsets=torch.tensor(off, dtype=torch.int32, device=DEV))


def dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def launch(z, t, w, off, tt, alpha=1.0, mu=1.0, norm_t=None, norm=None, arena=None, totals=False, dlogits=True):
    """One engine.bce_tower call; every output as numpy (out3, out6, dlogits, per_tower, total6)."""
    T, n = len(off) - 1, len(z)
    if norm_t is None:
        norm_t = max(int((TR.towers_ref(z, off, t, tt, w)["counted"] > 0).sum()), 1) if w is not None else T
    if arena is None:
        sc = E.TowerLossScratch(DEV, totals=totals)
        per = torch.empty(T, dtype=torch.float32, device=DEV)
        dz = None
        zd, td, wd, ttd, b = dev(z), dev(t), dev(w), dev(tt), fake_batch(off)
    else:
        nbytes = int(_lib.lib().spwgnn_bce_tower_scratch_bytes(n, T))
        sc = types.SimpleNamespace(scratch=arena.alloc(nbytes, torch.uint8, name="scratch"),
                                   out3=arena.alloc(3, torch.float32, 4, "out3", written=True),
                                   out6=arena.alloc(6, torch.float32, 4, "out6", written=True),
                                   total6=arena.put(np.zeros(6), 8, "total6", frozen=False) if totals else None,
                                   weights6=arena.put(np.full(6, 2.0), 8, "weights6") if totals else None)
        per = arena.alloc(T, torch.float32, 4, "per_tower", written=True)
        dz = arena.alloc(n, torch.float32, 4, "dlogits", written=True) if dlogits else None
        zd, td, wd, ttd = (None if a is None else arena.put(np.array(a), 4, nm) for a, nm in
                           ((z, "logits"), (t, "targets"), (w, "weights"), (tt, "tower_targets")))
        b = types.SimpleNamespace(n_nodes=n, n_towers=T, tower_nodes=np.diff(off),
                                  tower_offsets=arena.put(np.array(off, np.int32), 4, "tower_offsets"))
    out3, dz = E.bce_tower(zd, td, b, sc, mu, alpha, tower_targets=ttd, norm_t=norm_t, dlogits=dz, node_weights=wd,
                           norm=norm, total6=sc.total6, weights6=sc.weights6, per_tower=per, want_dlogits=dlogits)
    torch.cuda.synchronize()
    return types.SimpleNamespace(out3=out3.cpu().numpy(), out6=sc.out6.cpu().numpy(),
                                 dlogits=None if dz is None else dz.cpu().numpy(), per_tower=per.cpu().numpy(),
                                 total6=None if sc.total6 is None else sc.total6.cpu().numpy(), norm_t=norm_t)


def node_row(z, t, w):
    """spwgnn_bce / spwgnn_bce_weighted on the same inputs: (out3, dlogits) as numpy."""
    o3, dz = E.bce(dev(z), dev(t), E.BceScratch(DEV), node_weights=dev(w))
    torch.cuda.synchronize()
    return o3.cpu().numpy(), dz.cpu().numpy()


def bits(a):
    return np.asarray(a, np.float32).view(np.int32)


# -------------------------------------------------------------------------------- 1. the kernel against fp64
def test_cases_reach_every_branch():
    """What the docstring promises of the inputs (CPU only): both labels, s_u below the lower clip, above the
    upper one and inside, and both branches of log1mexp under T_u = 0."""
    for name in ("two_ragged257", "two_257x32", "two_65537x1"):
        z, t, w, off, tt = case(name)
        for tt_ in (None, tt):
            tw = TR.towers_ref(z, off, t, tt_, None)
            assert 0 < tw["T"].sum() < len(tw["T"]) and tw["inside"].any(), name
            if name == "two_65537x1":      # one node: z > 16.1 puts P_u above the upper clip
                assert (tw["s"] > TR.HI).any(), name
            else:                          # many nodes: P_u falls below the lower one
                assert (tw["s"] < TR.LO).any(), name
            zero = (tw["T"] == 0) & tw["inside"]
            assert (tw["s"][zero] > -TR.LN2).any() and (tw["s"][zero] < -TR.LN2).any(), name
    assert set(np.diff(case("two_ragged257")[3]).tolist()) >= set(range(1, 33))


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_kernel_against_fp64(name, weighted, explicit):
    """Per tower, l_u and every dlogit of the tower term against fp64, relative to (n_u + 16)·2^-24·max(1, |s_u|):
      * s_u is a sequential fp32 sum of n_u non-negative terms: (n_u − 1)u relative, plus each term's own error,
        <= 4u (expf, log1pf, the max and the add) — together (n_u + 3)u relative on s_u;
      * expm1f, logf / log1pf and the two divisions that turn s_u into l_u and g_u, the node's 1 / (1 + expf(z))
        and the products with mu and 1 / norm_t: <= 12u more;
      * with T_u = 0 the loss and g_u depend on s_u through exp(s_u), which turns the ABSOLUTE error of s_u,
        |s_u|·(n_u + 3)u, into a relative one: hence the factor max(1, |s_u|).
    (A numpy float32 emulation of the kernel's expressions on six of these shapes, every variant, stayed within
    0.32 of this bound.) Towers whose s_u lies within 1e-3 (relative) of a clip edge may fall on either side
    and are left out — at most 1 % of the towers, or the test fails (these inputs leave out 1 tower of 65,537). The tower term is isolated by alpha = 0; alpha in {1, 0.5}
    must then give fl(fl(alpha·d_node) + d_tower) exactly, d_node being spwgnn_bce(_weighted)'s dlogits."""
    z, t, w, off, tt = case(name)
    w_, tt_ = (w if weighted else None), (tt if explicit else None)
    mu = 0.75
    got = launch(z, t, w_, off, tt_, alpha=0.0, mu=mu)
    L, d_ref, tw = TR.tower_loss_ref(z, off, t, tt_, w_, mu, got.norm_t)
    sizes = np.diff(off)
    T = len(sizes)
    counted = tw["counted"] > 0
    keep = counted & ~tw["near_edge"]
    assert tw["near_edge"].sum() <= 0.01 * T, (name, int(tw["near_edge"].sum()))
    tol = (tw["counted"] + 16) * U * np.maximum(1.0, np.abs(tw["s"]))
    err = np.abs(got.per_tower - tw["loss"])
    assert np.all(err[keep] <= tol[keep] * np.abs(tw["loss"][keep])), (name, int(np.argmax(np.where(keep, err, 0))))
    assert np.all(got.per_tower[~counted] == 0)
    node_keep, node_tol = np.repeat(keep, sizes), np.repeat(tol, sizes)
    derr = np.abs(got.dlogits - d_ref)
    assert np.all(derr[node_keep] <= node_tol[node_keep] * np.abs(d_ref[node_keep])), (name, int(np.argmax(np.where(node_keep, derr, 0))))
    if weighted:
        assert np.all(bits(got.dlogits[w == 0]) == 0)                  # +0 for a masked node
    # the totals: each thread adds its towers (ceil(T / 65,536) of them) in fp32, then an 8-level fp32 tree, then
    # doubles and one division: the sum of non-negative terms to (ceil(T / 65,536) + 10)·u of the per-tower values
    assert got.out6[5] == counted.sum()
    psum = got.per_tower[counted].astype(np.float64).sum() / got.norm_t
    assert abs(got.out6[3] - psum) <= (-(-T // 65536) + 10) * U * abs(psum)
    # alpha = 0 with node targets: the node row is still reported, and stays out of the gradient
    n3, dn = node_row(z, t, w_)
    assert np.array_equal(bits(got.out6[:3]), bits(n3))
    assert got.out3[0] == np.float32(np.float64(mu) * np.float64(got.out6[3]))
    for alpha in (1.0, 0.5):
        comb = launch(z, t, w_, off, tt_, alpha=alpha, mu=mu)
        want = (np.float32(alpha) * dn).astype(np.float32) + got.dlogits
        assert np.array_equal(comb.dlogits, want.astype(np.float32)), (name, alpha)
        assert np.array_equal(bits(comb.out6), bits(got.out6))
        assert comb.out3[0] == np.float32(np.float64(np.float32(alpha)) * np.float64(got.out6[0]) + np.float64(mu) * np.float64(got.out6[3]))


def test_tower_accuracy_counts():
    """out6[4] against the reference where no node's probability is within the expf margin of 0.5."""
    import eval_ref as ER
    for name in ("one_ragged", "two_ragged257"):
        z, t, w, off, tt = case(name)
        z = np.where(ER.margin_ok(z, 0.5), z, np.float32(5.0))
        for w_, tt_ in ((None, None), (w, tt)):
            got = launch(z, t, w_, off, tt_)
            tw = TR.towers_ref(z, off, t, tt_, w_)
            assert got.out6[4] == (tw["correct"] & (tw["counted"] > 0)).sum() and got.out6[5] == (tw["counted"] > 0).sum()


def test_towers_well_outside_the_clip_have_zero_tower_gradient():
    """All z >= 20 (P_u above 1 − 1e-7) and 32-node towers of z = −1 (P_u below 1e-7), both labels: the tower
    term adds exactly nothing, the losses are the clipped ones."""
    z = np.concatenate([np.full(5, 20.0), np.linspace(20, 30, 7), np.full(64, -1.0)]).astype(np.float32)
    off = np.array([0, 5, 12, 44, 76], np.int32)
    tt = np.array([1, 0, 1, 0], np.float32)
    t = np.ones(76, np.float32)
    got = launch(z, t, None, off, tt, alpha=0.0, mu=2.0)
    assert np.all(bits(got.dlogits) == 0)
    lo, hi = np.float64(TR.LO), np.float64(TR.HI)
    want = np.array([-hi, -TR.log1mexp(hi), -lo, -TR.log1mexp(lo)])
    assert np.all(np.abs(got.per_tower - want) <= 4 * U * np.abs(want) + 2e-9)   # −log1mexp(lo) ≈ 1e-7: expf's ulp of 1e-7
    assert got.out6[5] == 4 and got.out6[4] == 2                                 # predicted stable: towers 0, 1


# -------------------------------------------------------------------------------- 2. bit contracts
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", ["one_ragged", "one_8x32", "two_ragged257", "two_257x32", "two_65537x1"])
def test_node_row_carries_the_bits_of_bce(name, weighted):
    z, t, w, off, tt = case(name)
    w_ = w if weighted else None
    n3, _ = node_row(z, t, w_)
    for tt_ in (None, tt):
        got = launch(z, t, w_, off, tt_, alpha=1.0, mu=0.5)
        assert np.array_equal(bits(got.out6[:3]), bits(n3)) and np.array_equal(bits(got.out3[1:]), bits(n3[1:]))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("T", [8, 300])
def test_dlogits_equal_bce_when_every_tower_is_outside_the_clip(T, weighted):
    """32-node towers of z ~ N(−1, 0.3): s_u ≈ −42 < log(1e-7) for every tower (asserted on the reference),
    alpha = 1: dlogits carry spwgnn_bce(_weighted)'s bits."""
    rng = np.random.default_rng(T)
    n = 32 * T
    z = rng.normal(-1.0, 0.3, n).astype(np.float32)
    t = rng.integers(0, 2, n).astype(np.float32)
    w = rng.choice(np.array([0.5, 1.0, 2.5], np.float32), n) if weighted else None   # no zeros: every node counts
    off = (np.arange(T + 1) * 32).astype(np.int32)
    assert not TR.towers_ref(z, off, t, None, w)["inside"].any()
    n3, dn = node_row(z, t, w)
    got = launch(z, t, w, off, None, alpha=1.0, mu=3.0)
    assert np.array_equal(bits(got.dlogits), bits(dn)) and np.array_equal(bits(got.out6[:3]), bits(n3))


@pytest.mark.parametrize("name", ["one_ragged", "two_ragged257"])
def test_device_divisors_equal_value_divisors_and_runs_repeat(name):
    z, t, w, off, tt = case(name)
    norm, norm_t = float(max(np.count_nonzero(w), 1)), 37.0
    a = launch(z, t, w, off, tt, alpha=0.5, mu=0.25, norm=norm, norm_t=norm_t, totals=True)
    b = launch(z, t, w, off, tt, alpha=0.5, mu=0.25, norm=dev([norm]), norm_t=dev([norm_t]), totals=True)
    c = launch(z, t, w, off, tt, alpha=0.5, mu=0.25, norm=norm, norm_t=norm_t, totals=True)
    for x in (b, c):
        for k in ("out3", "out6", "dlogits", "per_tower"):
            assert np.array_equal(bits(getattr(a, k)), bits(getattr(x, k))), k
        assert np.array_equal(a.total6, x.total6)
    assert np.array_equal(a.total6, a.out6.astype(np.float64))          # weights6 of ones, from zero


# -------------------------------------------------------------------------------- 3. masks
@pytest.mark.parametrize("name", ["one_ragged", "two_ragged257"])
def test_masked_nodes_reach_nothing(name):
    z, t, w, off, tt = case(name)
    w = w.copy()
    w[off[2]:off[3]] = 0.0                                  # one tower fully masked
    w[off[4]] = 1.0
    zn, tn = z.copy(), t.copy()
    zn[w == 0], tn[w == 0] = np.nan, np.nan
    for tt_ in (None, tt):
        a = launch(z, t, w, off, tt_, alpha=1.0, mu=1.0)
        b = launch(zn, tn, w, off, tt_, alpha=1.0, mu=1.0)
        for k in ("out3", "out6", "dlogits", "per_tower"):
            assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
        assert np.isfinite(a.out3).all() and np.all(bits(a.dlogits[w == 0]) == 0)
        counted = TR.towers_ref(z, off, t, tt_, w)["counted"] > 0
        assert not counted[2] and a.out6[5] == counted.sum() < len(off) - 1 and a.per_tower[2] == 0
    # tower-only labels: no node targets at all
    c = launch(z, None, w, off, tt, alpha=0.0, mu=1.0)
    d = launch(z, t, w, off, tt, alpha=0.0, mu=1.0)
    assert np.array_equal(bits(c.dlogits), bits(d.dlogits)) and np.array_equal(bits(c.out6[3:]), bits(d.out6[3:]))
    assert np.array_equal(c.out6[:3], [0, 0, np.count_nonzero(w)]) and c.out3[0] == d.out3[0]
    e = launch(z, None, None, off, tt, alpha=0.0, mu=1.0)
    assert np.array_equal(e.out6[:3], [0, 0, len(z)])


# -------------------------------------------------------------------------------- 4. agreement with evaluate
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", ["one_ragged", "two_ragged257", "two_257x32"])
def test_tower_accuracy_equals_evaluates_tower_table(name, weighted):
    z, t, w, off, tt = case(name)
    w_ = w if weighted else None
    got = launch(z, t, w_, off, None)
    tables = E.EvalTables(DEV)
    E.eval_metrics(dev(z), dev(t), tables, batch=fake_batch(off), node_weights=dev(w_), threshold=0.5)
    t6 = tables.cpu()["tower6"][0]
    assert got.out6[4] == t6[2] + t6[3] and got.out6[5] == t6[0] and t6[0] > 0


# -------------------------------------------------------------------------------- 7. guard bands
@pytest.mark.parametrize("weighted,explicit", [(False, False), (True, True)])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_guard_bands(name, weighted, explicit):
    z, t, w, off, tt = case(name)
    arena = G.Arena(DEV)
    got = launch(z, t, w if weighted else None, off, tt if explicit else None, alpha=0.5, mu=0.5, arena=arena, totals=True)
    arena.check(name)
    assert np.array_equal(got.total6, 2.0 * got.out6.astype(np.float64))
    ref = launch(z, t, w if weighted else None, off, tt if explicit else None, alpha=0.5, mu=0.5)
    for k in ("out3", "out6", "dlogits", "per_tower"):                    # odd alignment changes nothing
        assert np.array_equal(bits(getattr(got, k)), bits(getattr(ref, k))), k


def test_guard_bands_loss_only():
    z, t, w, off, tt = case("two_ragged257")
    arena = G.Arena(DEV)
    got = launch(z, None, w, off, tt, alpha=0.0, mu=1.0, arena=arena, dlogits=False)
    arena.check("loss only")
    assert got.dlogits is None and np.isfinite(got.out6).all()
