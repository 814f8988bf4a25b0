"""TowerBatch: the reference's 4-tensor input dict, compacted for the HIP kernels.

The reference feeds Keras (B, N, 3) objects, two dense (B, N, E) one-hot relation matrices and a
(B, N, 100) propagation state (src/Networks.py:22-29; built by src/main.py:66-93). Every active
relation column is one sender and one receiver, so the batch becomes a union graph: node rows
(objects, propagation) and an edge list, packed by the C library into wave-tiles of whole towers
and 32-edge blocks (spwgnn_plan_size/fill). Conversion happens once per batch on the host (C++);
the device arrays then stay resident in HBM.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import _lib


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


SMALL_BATCH_TOWERS = 2048   # below this a batch cannot fill the chip's 2,048 edge waves anyway


def default_nw_max(max_nodes: int, n_towers: int = 1 << 30) -> int:
    """Nodes per wave-tile: at least one whole tower. Up to 16 nodes the backward segment sums run
    as one one-hot matrix product (receiver rows 0-15, sender rows 16-31), so small towers are
    packed up to 16 nodes per wave; larger towers take one wave-tile each (≤ 32 nodes). A small
    batch (fewer towers than the edge kernels have waves) takes one tower per wave-tile instead:
    each wave then walks one tower's blocks, not two or three, which is the step's latency at
    batch 32 (the reference's fit, main.py:92-98)."""
    if max_nodes > 16:
        return int(min(_NW_LIMIT, max_nodes))
    return max(int(max_nodes), 1) if n_towers < SMALL_BATCH_TOWERS else 16


_NW_LIMIT = 32


def upload(arrays, device) -> list:
    """Host arrays → device tensors in ONE copy: packed (16-byte aligned) into a pinned staging
    buffer and copied with non_blocking=True, so the host does not wait for the stream to drain (a
    copy from pageable memory does) and can build the next batch while the GPU runs this one. The
    caching host allocator keeps the staging block until its copy has run."""
    dev = torch.device(device)
    arrays = [np.ascontiguousarray(a) for a in arrays]
    if dev.type != "cuda":
        return [torch.from_numpy(a.copy()) for a in arrays]
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 15) // 16 * 16
    host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    for a, o in zip(arrays, offs):
        hv[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    d = host.to(dev, non_blocking=True)
    out = []
    for a, o in zip(arrays, offs):
        t = d[o:o + a.nbytes].view(torch.from_numpy(a[:0].reshape(-1)).dtype) if a.nbytes else \
            torch.empty(0, dtype=torch.from_numpy(a[:0].reshape(-1)).dtype, device=dev)
        out.append(t.view(a.shape))
    return out


def pack_order(tower_nodes, tower_edges, nw_max: int = 16) -> np.ndarray:
    """spwgnn_plan_order: a tower order that packs a ragged batch into fewer 32-edge blocks (towers by
    decreasing edge count into the wave-tile whose last block has room; include/spwgnn.h)."""
    tn = np.ascontiguousarray(tower_nodes, dtype=np.int32)
    te = np.ascontiguousarray(tower_edges, dtype=np.int32)
    order = np.zeros(len(tn), np.int32)
    if len(tn):
        _lib.check(_lib.lib().spwgnn_plan_order(len(tn), _ptr(tn), _ptr(te), int(nw_max), _ptr(order)), "plan_order")
    return order


def reorder_towers(pos, tower_nodes, src, dst, tower_edges, order, prop=None):
    """The towers of a compact edge-form batch in `order` (order[k] = the k-th tower): node rows,
    edges (node ids rebased), counts. Returns (pos, tower_nodes, src, dst, tower_edges, prop, node_perm)
    with node_perm[i] = the input-order index of node i of the reordered batch."""
    tn = np.asarray(tower_nodes, np.int64)
    te = np.asarray(tower_edges, np.int64)
    order = np.asarray(order, np.int64)
    noff = np.concatenate([[0], np.cumsum(tn)])
    eoff = np.concatenate([[0], np.cumsum(te)])
    node_perm = np.concatenate([np.arange(noff[t], noff[t + 1]) for t in order]) if len(order) else np.zeros(0, np.int64)
    edge_perm = np.concatenate([np.arange(eoff[t], eoff[t + 1]) for t in order]) if len(order) else np.zeros(0, np.int64)
    new_noff = np.concatenate([[0], np.cumsum(tn[order])])
    shift = np.repeat(new_noff[:-1] - noff[order], te[order])     # per reordered edge: old → new node base
    src = np.asarray(src, np.int64)[edge_perm] + shift
    dst = np.asarray(dst, np.int64)[edge_perm] + shift
    pos = np.asarray(pos)[node_perm]
    prop = None if prop is None else np.asarray(prop).reshape(int(noff[-1]), -1)[node_perm]
    return (pos, tn[order].astype(np.int32), src.astype(np.int32), dst.astype(np.int32), te[order].astype(np.int32),
            prop, node_perm)


@dataclass
class HostPlan:
    """A batch's host-side arrays in upload order (pos4, node_tower, node_local, wtile, edge_src,
    edge_dst, blk_csr[, prop]) plus the sizes the kernels are launched with."""
    n_towers: int
    n_nodes: int
    tower_nodes: np.ndarray
    tower_edges: np.ndarray
    src: np.ndarray
    dst: np.ndarray
    n_wtiles: int
    n_eblocks: int
    nw_max: int
    edge_id: np.ndarray
    node_shape: Optional[tuple]
    has_prop: bool
    arrays: list
    flags: int = 0     # spwgnn_batch.flags (_lib.BATCH_RECV_BLOCKS: a receiver-block plan)
    node_perm: Optional[np.ndarray] = None   # packed plans: node i of the plan = input node node_perm[i]

    @property
    def geometry(self) -> tuple:
        """What a captured step bakes in: sizes, layout flags and every array's shape."""
        return (self.n_towers, self.n_nodes, self.n_wtiles, self.n_eblocks, self.nw_max, self.has_prop, self.flags,
                tuple(a.shape for a in self.arrays))

    def edges_to_input(self, values, dense: bool = False):
        """`TowerBatch.edges_to_input` of the batch this plan becomes (it reads the host fields they share)."""
        return TowerBatch.edges_to_input(self, values, dense)

    def edge_gates(self, values, fill: float = 0.0, device=None) -> torch.Tensor:
        """`TowerBatch.edge_gates` of the batch this plan becomes, on ``device`` (default: where ``values`` is)."""
        return TowerBatch.edge_gates(self, values, fill, device)

    def edge_step_gates(self, values, fill: float = 0.0, device=None) -> torch.Tensor:
        """`TowerBatch.edge_step_gates` of the batch this plan becomes."""
        return TowerBatch.edge_step_gates(self, values, fill, device)

    @staticmethod
    def build(pos, tower_nodes, src, dst, tower_edges, prop=None, nw_max=None, node_shape=None, tower_ids=None,
              edge_cap=None, recv_blocks=None, pack: bool = False) -> "HostPlan":
        """recv_blocks: one 32-edge block per node holding its in-edges (spwgnn_plan_fill_recv; the x6
        edge forward then sums a node's messages as a column sum). None = automatic: for wave-tiles of
        more than 16 nodes whose blocks would be ≥ 80 % full (large, densely connected towers —
        BASELINE config 5), never with edge_cap.
        pack: plan the towers in spwgnn_plan_order's order (ragged batches: fewer, fuller blocks). Each
        tower keeps its id (dropout key) and `node_perm` maps the plan's node rows back to the input's:
        logits and d/d'propagation' come out in plan order (TowerBatch.to_input_order), targets go in
        in plan order (TowerBatch.to_plan_order)."""
        if pack:
            tn0 = np.asarray(tower_nodes, np.int32)
            if nw_max is None:
                nw_max = default_nw_max(int(tn0.max()) if len(tn0) else 1, len(tn0))
            order = pack_order(tn0, tower_edges, min(int(nw_max), 16) if int(tn0.max()) <= 16 else int(nw_max))
            tid0 = np.arange(len(tn0), dtype=np.int64) if tower_ids is None else np.asarray(tower_ids, np.int64)
            pos, tower_nodes, src, dst, tower_edges, prop, perm = reorder_towers(pos, tn0, src, dst, tower_edges, order,
                                                                                prop)
            cap = None if edge_cap is None else np.broadcast_to(np.asarray(edge_cap, np.int32), (len(tn0),))[order]
            plan = HostPlan.build(pos, tower_nodes, src, dst, tower_edges, prop, nw_max, None, tid0[order], cap,
                                  recv_blocks)
            plan.node_perm = perm
            return plan
        L = _lib.lib()
        tower_nodes = np.ascontiguousarray(tower_nodes, dtype=np.int32)
        tower_edges = np.ascontiguousarray(tower_edges, dtype=np.int32)
        src = np.ascontiguousarray(src, dtype=np.int32)
        dst = np.ascontiguousarray(dst, dtype=np.int32)
        T = len(tower_nodes)
        Nn = int(tower_nodes.sum())
        if T == 0:
            raise ValueError("empty batch: at least one tower is needed")
        if pos.shape[0] != Nn:
            raise ValueError(f"pos has {pos.shape[0]} rows, towers hold {Nn} nodes")
        if int(tower_edges.sum()) != len(src) or len(src) != len(dst):
            raise ValueError("edge counts do not match the edge list")
        if nw_max is None:
            nw_max = default_nw_max(int(tower_nodes.max()) if T else 1, T)
        if T and int(tower_nodes.max()) > _NW_LIMIT:
            raise ValueError(f"towers of more than {_NW_LIMIT} nodes are not supported by this build")
        if recv_blocks is None:
            recv_blocks = (edge_cap is None and nw_max > 16 and len(src) > 0 and Nn * 32 <= 1.25 * len(src)
                           and int(np.bincount(dst, minlength=Nn).max()) <= 32)
        if recv_blocks and edge_cap is not None:
            raise ValueError("receiver-block plans do not take edge capacities")
        cap = None
        if edge_cap is not None:
            cap = np.ascontiguousarray(np.broadcast_to(np.asarray(edge_cap, np.int32), (T,)), dtype=np.int32)
            if np.any(cap < tower_edges):
                raise ValueError("edge_cap must be >= every tower's edge count")
        sizes = _lib.PlanSizes()
        if recv_blocks:
            _lib.check(L.spwgnn_plan_size_recv(T, _ptr(tower_nodes), nw_max, C.byref(sizes)), "plan_size_recv")
        elif cap is None:
            _lib.check(L.spwgnn_plan_size(T, _ptr(tower_nodes), _ptr(tower_edges), nw_max, C.byref(sizes)), "plan_size")
        else:
            _lib.check(L.spwgnn_plan_size_cap(T, _ptr(tower_nodes), _ptr(cap), nw_max, C.byref(sizes)), "plan_size_cap")
        wtile = np.zeros((sizes.n_wtiles, 4), np.int32)
        esrc = np.zeros(sizes.n_eblocks * 32, np.int32)
        edst = np.zeros(sizes.n_eblocks * 32, np.int32)
        eid = np.zeros(sizes.n_eblocks * 32, np.int32)
        csr = np.zeros((sizes.n_eblocks, 128), np.uint8)
        sp = _ptr(src) if len(src) else None
        dp = _ptr(dst) if len(dst) else None
        if recv_blocks:
            _lib.check(L.spwgnn_plan_fill_recv(T, _ptr(tower_nodes), _ptr(tower_edges), sp, dp, nw_max, C.byref(sizes),
                                               _ptr(wtile), _ptr(esrc), _ptr(edst), _ptr(eid), _ptr(csr)), "plan_fill_recv")
        elif cap is None:
            _lib.check(L.spwgnn_plan_fill(T, _ptr(tower_nodes), _ptr(tower_edges), sp, dp, nw_max, C.byref(sizes),
                                          _ptr(wtile), _ptr(esrc), _ptr(edst), _ptr(eid), _ptr(csr)), "plan_fill")
        else:
            _lib.check(L.spwgnn_plan_fill_cap(T, _ptr(tower_nodes), _ptr(tower_edges), _ptr(cap), sp, dp, nw_max,
                                              C.byref(sizes), _ptr(wtile), _ptr(esrc), _ptr(edst), _ptr(eid),
                                              _ptr(csr)), "plan_fill_cap")
        tid = np.arange(T, dtype=np.int32) if tower_ids is None else np.asarray(tower_ids, np.int64)
        if len(tid) != T or (T and (tid.min() < 0 or tid.max() > np.iinfo(np.int32).max)):
            raise ValueError("tower_ids must hold one non-negative int32 id per tower")
        node_tower = np.repeat(tid.astype(np.int32), tower_nodes)
        starts = np.concatenate([[0], np.cumsum(tower_nodes)[:-1]]).astype(np.int64)
        node_local = (np.arange(Nn) - np.repeat(starts, tower_nodes)).astype(np.int32)
        pos4 = np.zeros((Nn, 4), np.float32)
        pos4[:, :3] = np.asarray(pos, np.float32)[:, :3]
        host = [pos4, node_tower, node_local, wtile, esrc, edst, csr]
        if prop is not None:
            host.append(np.asarray(prop, np.float32).reshape(Nn, 100))
        return HostPlan(T, Nn, tower_nodes, tower_edges, src, dst, sizes.n_wtiles, sizes.n_eblocks, sizes.nw_max,
                        eid, node_shape, prop is not None, host, _lib.BATCH_RECV_BLOCKS if recv_blocks else 0)


@dataclass
class TowerBatch:
    n_towers: int
    n_nodes: int
    tower_nodes: np.ndarray          # (T,) int32
    tower_edges: np.ndarray          # (T,) int32 active relations per tower
    src: np.ndarray                  # (Ne,) int32 global sender (host copy)
    dst: np.ndarray                  # (Ne,) int32 global receiver
    n_wtiles: int
    n_eblocks: int
    nw_max: int
    device: torch.device
    pos: torch.Tensor                # (Nn, 4) f32
    prop: Optional[torch.Tensor]     # (Nn, 100) f32 or None (= zeros)
    node_tower: torch.Tensor
    node_local: torch.Tensor
    wtile: torch.Tensor
    edge_src: torch.Tensor
    edge_dst: torch.Tensor
    blk_csr: torch.Tensor
    edge_id: np.ndarray              # (n_eblocks*32,) original edge index or -1
    node_shape: Optional[tuple] = None   # (B, N) when built from a uniform-N dense batch
    flags: int = 0                       # spwgnn_batch.flags (the plan's layout)
    node_perm: Optional[np.ndarray] = None   # packed plans (HostPlan.build pack=True): plan node i = input node node_perm[i]
    _cstruct: Optional[_lib.BatchC] = field(default=None, repr=False)

    generation = 0   # refills of a device-built batch (DeviceTowerBatch.refill); part of engine.Workspace.key

    def to_plan_order(self, x):
        """Per-node rows (targets, propagation) in the input's node order → the plan's (identity
        unless the plan was packed). numpy or torch, first axis = nodes."""
        if self.node_perm is None:
            return x
        if isinstance(x, torch.Tensor):
            return x[torch.as_tensor(self.node_perm, device=x.device)]
        return np.asarray(x)[self.node_perm]

    def to_input_order(self, x):
        """Per-node results (logits, d/d'propagation') in the plan's node order → the input's."""
        if self.node_perm is None:
            return x
        if isinstance(x, torch.Tensor):
            out = torch.empty_like(x)
            out[torch.as_tensor(self.node_perm, device=x.device)] = x
            return out
        out = np.empty_like(np.asarray(x))
        out[self.node_perm] = x
        return out

    def towers_to_plan_order(self, x):
        """Per-tower rows (tower targets) in the input's tower order → the plan's (identity unless the plan
        was packed). Plan tower t starts at input node node_perm[offset_t]; the input's towers start at
        increasing nodes, so the rank of that node among the towers' first nodes is the input tower."""
        if self.node_perm is None:
            return x
        tn = np.asarray(self.tower_nodes, np.int64)
        if np.any(tn < 1):
            raise ValueError("a packed plan with an empty tower has no tower order")
        first = np.asarray(self.node_perm)[np.concatenate([[0], np.cumsum(tn)[:-1]])]
        order = np.argsort(np.argsort(first, kind="stable"), kind="stable")
        if isinstance(x, torch.Tensor):
            return x[torch.as_tensor(order, device=x.device)]
        return np.asarray(x)[order]

    def edges_to_input(self, values, dense: bool = False):
        """Per-edge-slot results (`engine.backward_relations`: last axis = the plan's 32·n_eblocks edge
        slots, numpy or torch, any leading axes such as the steps) → ``(src, dst, values)`` with the padding
        slots dropped: edge j is the j-th active relation (the order of ``self.src`` / ``self.dst``:
        tower-major, inside a tower the order the list was given in), its node ids in the INPUT's node order (through
        ``node_perm`` for packed plans), values[..., j] its value. With ``dense`` (towers of one size N
        only) instead one (..., B, N, N) array indexed [tower, sender, receiver] in the input's tower
        order, zero where there is no relation; a pair that appears twice in the edge list has two values
        and one cell, so the dense form raises ValueError naming it (the 1-D form returns both)."""
        eid = np.asarray(self.edge_id)
        v = values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else np.asarray(values)
        if v.shape[-1] != len(eid):
            raise ValueError(f"values must hold one entry per edge slot ({len(eid)}), got {v.shape}")
        slots = np.nonzero(eid >= 0)[0]
        slots = slots[np.argsort(eid[slots], kind="stable")]   # the slot of edge j
        src, dst = np.asarray(self.src, np.int64), np.asarray(self.dst, np.int64)
        if self.node_perm is not None:
            perm = np.asarray(self.node_perm, np.int64)
            src, dst = perm[src], perm[dst]
        vals = v[..., slots]
        if not dense:
            return src, dst, vals
        tn = np.asarray(self.tower_nodes)
        if len(tn) == 0 or np.any(tn != tn[0]):
            raise ValueError("the dense form needs towers of one size")
        N = int(tn[0])
        cell, first, count = np.unique(src * N + dst % N, return_index=True, return_counts=True)
        if len(cell) < len(src):   # a repeated pair: one cell cannot hold two values
            k = int(np.argmax(count > 1))
            j = int(first[k])
            raise ValueError(f"the dense form has one cell per (tower, sender, receiver): relation {int(src[j]) % N} -> "
                             f"{int(dst[j]) % N} of tower {int(src[j]) // N} appears {int(count[k])} times; use the "
                             "1-D form")
        out = np.zeros(v.shape[:-1] + (len(tn), N, N), v.dtype)
        out[..., src // N, src % N, dst % N] = vals
        return out

    def edge_gates(self, values, fill: float = 0.0, device=None) -> torch.Tensor:
        """Per-relation values → the (32·n_eblocks,) fp32 tensor in the plan's edge-slot order that
        ``engine.forward(..., gates=)`` takes: the inverse of `edges_to_input`. ``values`` is a 1-D tensor with
        one entry per active relation in the input's edge order (the order of ``self.src`` / ``self.dst``), or,
        for towers of one size N, a dense (B, N, N) tensor indexed [tower, sender, receiver] in the input's
        tower and node order (through ``node_perm`` for packed plans); entries without a relation are not read.
        Padding slots get ``fill`` (the engine never reads them). Built from torch indexing ops on the
        batch's device, so autograd reaches ``values``."""
        dev = getattr(self, "device", None) if device is None else torch.device(device)
        v = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values))
        if dev is None:
            dev = v.device
        v = v.to(device=dev, dtype=torch.float32)
        eid = np.asarray(self.edge_id, np.int64)
        src, dst = np.asarray(self.src, np.int64), np.asarray(self.dst, np.int64)
        if v.dim() == 1:
            if v.shape[0] != len(src):
                raise ValueError(f"values must hold one entry per active relation ({len(src)}), got {tuple(v.shape)}")
            pick = np.maximum(eid, 0)
        elif v.dim() == 3:
            tn = np.asarray(self.tower_nodes)
            if len(tn) == 0 or np.any(tn != tn[0]) or tuple(v.shape) != (len(tn), int(tn[0]), int(tn[0])):
                raise ValueError("the dense form needs towers of one size N and a (B, N, N) [tower, sender, receiver] "
                                 f"tensor, got {tuple(v.shape)}")
            N = int(tn[0])
            if self.node_perm is not None:
                perm = np.asarray(self.node_perm, np.int64)
                src, dst = perm[src], perm[dst]
            flat = src * N + dst % N   # ((b·N + s)·N + r) with src = b·N + s
            pick = flat[np.maximum(eid, 0)] if len(flat) else np.zeros(len(eid), np.int64)
            v = v.reshape(-1)
        else:
            raise ValueError(f"values must be 1-D (input edge order) or (B, N, N), got {tuple(v.shape)}")
        if v.numel() == 0:
            return torch.full((len(eid),), float(fill), dtype=torch.float32, device=dev)
        active = torch.as_tensor(eid >= 0, device=dev)
        got = v[torch.as_tensor(pick, device=dev)]
        return torch.where(active, got, torch.full_like(got, float(fill))).contiguous()

    def edge_step_gates(self, values, fill: float = 0.0, device=None) -> torch.Tensor:
        """Per-relation, per-step values → the (S, 32·n_eblocks) fp32 tensor that ``engine.forward(...,
        step_gates=)`` takes: row s is `edge_gates` of ``values[s]``. ``values`` is (S, E) in the input's edge
        order, or (S, B, N, N) indexed [step, tower, sender, receiver] for towers of one size (through
        ``node_perm`` for packed plans). Built from torch indexing ops, so autograd reaches ``values``."""
        v = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values))
        if v.dim() not in (2, 4) or v.shape[0] < 1:
            raise ValueError(f"values must be (S, E) in the input's edge order or (S, B, N, N), got {tuple(v.shape)}")
        return torch.stack([self.edge_gates(v[s], fill, device) for s in range(v.shape[0])]).contiguous()

    @property
    def n_edges(self) -> int:
        return int(len(self.src))

    @property
    def tower_offsets(self) -> torch.Tensor:
        """(T+1,) int32 device node offsets of the towers (built on first use)."""
        t = getattr(self, "_tower_offsets", None)
        if t is None:
            off = np.concatenate([[0], np.cumsum(self.tower_nodes)]).astype(np.int32)
            t = torch.from_numpy(off).to(self.device)
            object.__setattr__(self, "_tower_offsets", t)
        return t

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_edges(pos: np.ndarray, tower_nodes, src, dst, tower_edges, prop=None, device="cuda",
                   nw_max: Optional[int] = None, node_shape=None, tower_ids=None, edge_cap=None,
                   recv_blocks=None, pack: bool = False) -> "TowerBatch":
        """pos (Nn, >=3) objects rows (already /170); towers are consecutive node ranges;
        edges tower-major with global node ids. `tower_ids` (T,): each tower's index in the batch it
        was cut from (the dropout masks are keyed by it), so a shard or micro-batch of a larger batch
        draws the masks the whole batch would; default 0..T-1. `edge_cap` (T,) ≥ tower_edges: size
        each tower's blocks for that many edges (spwgnn_plan_fill_cap) so same-shape batches share
        one plan geometry (replayed hipGraph steps); default: the actual edge counts."""
        plan = HostPlan.build(pos, tower_nodes, src, dst, tower_edges, prop, nw_max, node_shape, tower_ids, edge_cap,
                              recv_blocks, pack)
        return TowerBatch.from_plan(plan, device)

    @staticmethod
    def from_plan(plan: "HostPlan", device, dev_arrays: Optional[list] = None) -> "TowerBatch":
        """A device batch from a host plan: its arrays uploaded in one copy, or `dev_arrays` (device
        tensors of the plan's array shapes, e.g. a replayed step's static buffers) used as they are."""
        dev = torch.device(device)
        d = dev_arrays if dev_arrays is not None else upload(plan.arrays, dev)
        m = plan
        prop_t = d[7] if m.has_prop else None
        return TowerBatch(m.n_towers, m.n_nodes, m.tower_nodes, m.tower_edges, m.src, m.dst, m.n_wtiles, m.n_eblocks,
                          m.nw_max, dev, d[0], prop_t, d[1], d[2], d[3], d[4], d[5], d[6], m.edge_id, m.node_shape,
                          m.flags, m.node_perm)

    @staticmethod
    def from_dense(objects, sender_relations, receiver_relations, propagation=None, device="cuda",
                   nw_max: Optional[int] = None) -> "TowerBatch":
        """The reference input dict (Networks.py:22-29) → compact batch (C++ conversion)."""
        to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        obj = np.ascontiguousarray(to_np(objects), np.float32)
        Rs = np.ascontiguousarray(to_np(sender_relations), np.float32)
        Rr = np.ascontiguousarray(to_np(receiver_relations), np.float32)
        B, N = obj.shape[:2]
        E = N * (N - 1)
        if Rs.shape != (B, N, E) or Rr.shape != (B, N, E):
            raise ValueError(f"relation matrices must be (B, N, N(N-1)) = {(B, N, E)}; got {Rs.shape}, {Rr.shape}")
        L = _lib.lib()
        cap = B * E
        src = np.zeros(max(cap, 1), np.int32)
        dst = np.zeros(max(cap, 1), np.int32)
        tec = np.zeros(B, np.int32)
        ne = C.c_int64(0)
        _lib.check(L.spwgnn_dense_to_edges(_ptr(Rs), _ptr(Rr), B, N, _ptr(src), _ptr(dst), None, cap, C.byref(ne),
                                           _ptr(tec)), "dense_to_edges")
        n = int(ne.value)
        prop = None
        if propagation is not None:
            p = to_np(propagation)
            if np.any(p != 0):
                prop = np.asarray(p, np.float32).reshape(B * N, 100)
        return TowerBatch.from_edges(obj.reshape(B * N, 3), np.full(B, N, np.int32), src[:n], dst[:n], tec, prop,
                                     device, nw_max, node_shape=(B, N))

    @staticmethod
    def fully_connected(objects: np.ndarray, propagation=None, device="cuda", nw_max=None,
                        tower_ids=None, recv_blocks=None) -> "TowerBatch":
        """Fast path for (B, N, 3) towers whose relations are all active (the inference relation
        set of JengaBuilder.py:309-326 and the benchmark configs)."""
        obj = np.asarray(objects, np.float32)
        B, N = obj.shape[:2]
        m_idx, j_idx = np.nonzero(~np.eye(N, dtype=bool))
        base = (np.arange(B, dtype=np.int64) * N)[:, None]
        src = (base + m_idx[None, :]).reshape(-1).astype(np.int32)
        dst = (base + j_idx[None, :]).reshape(-1).astype(np.int32)
        prop = None if propagation is None else np.asarray(propagation, np.float32).reshape(B * N, 100)
        return TowerBatch.from_edges(obj.reshape(B * N, 3), np.full(B, N, np.int32), src, dst,
                                     np.full(B, N * (N - 1), np.int32), prop, device, nw_max, node_shape=(B, N),
                                     tower_ids=tower_ids, recv_blocks=recv_blocks)

    @staticmethod
    def ragged(objects_list, relation_threshold: Optional[float] = None, device="cuda", nw_max=None,
               raw_positions_list=None) -> "TowerBatch":
        """Towers of different sizes: list of (N_b, 3) objects; relations fully connected, or
        thresholded on ``raw_positions_list`` (pixels) like main.py:71-81."""
        if len(objects_list) == 0:
            raise ValueError("empty batch: at least one tower is needed")
        tower_nodes = np.array([len(o) for o in objects_list], np.int32)
        srcs, dsts, tes = [], [], []
        off = 0
        for b, o in enumerate(objects_list):
            N = len(o)
            m_idx, j_idx = np.nonzero(~np.eye(N, dtype=bool))
            if relation_threshold is not None:
                raw = np.asarray(raw_positions_list[b])
                keep = np.linalg.norm(raw[m_idx, 0:2] - raw[j_idx, 0:2], axis=1) < relation_threshold
                m_idx, j_idx = m_idx[keep], j_idx[keep]
            srcs.append(off + m_idx)
            dsts.append(off + j_idx)
            tes.append(len(m_idx))
            off += N
        src = np.concatenate(srcs).astype(np.int32) if srcs else np.zeros(0, np.int32)
        dst = np.concatenate(dsts).astype(np.int32) if dsts else np.zeros(0, np.int32)
        pos = np.concatenate([np.asarray(o, np.float32) for o in objects_list], axis=0)
        return TowerBatch.from_edges(pos, tower_nodes, src, dst, np.array(tes, np.int32), None, device, nw_max)

    # ------------------------------------------------------------------ plans built on the device
    @staticmethod
    def from_positions(raw: torch.Tensor, threshold: Optional[float] = 170.0, divisor: float = 170.0,
                       tower_nodes=None, nw_max: Optional[int] = None, edge_cap=None, tower_ids=None,
                       propagation: Optional[torch.Tensor] = None, check: bool = False) -> "DeviceTowerBatch":
        """Raw-pixel positions on the device → batch, without a host round trip: ``raw`` (B, N, ≥3) or,
        with ``tower_nodes`` (T,), (n_nodes, ≥3) rows [x, y, w] of consecutive ragged towers. The
        relation set is the reference's thresholded one (raw-pixel distance < ``threshold``,
        main.py:71-81; None, ≤ 0 or NaN: fully connected, JengaBuilder.py:309-326) and the node rows are
        raw / ``divisor`` (main.py:91), both computed by one kernel (spwgnn_plan_device_positions) on a
        capacity plan whose geometry is cached per shape (`plan_geometry`). ``edge_cap``: relations each
        tower's blocks are sized for (default N(N−1), every slot; a lower cap gives fewer padding blocks
        and is guarded by the status word). ``check=False`` never synchronises: the status stays on the
        device as ``batch.status``; ``check=True`` reads it and raises `SpwgnnError` on an error."""
        raw = _device_f32(raw, "raw")
        if raw.dim() == 3 and tower_nodes is None:
            B, N = int(raw.shape[0]), int(raw.shape[1])
            tn, node_shape = _Uniform(B, N), (B, N)
        elif raw.dim() == 2 and tower_nodes is not None:
            tn, node_shape = np.ascontiguousarray(tower_nodes, dtype=np.int32), None
        else:
            raise ValueError("raw must be (B, N, 3), or (n_nodes, 3) with tower_nodes")
        rows = raw.reshape(-1, raw.shape[-1])
        if rows.shape[1] < 3:
            raise ValueError("raw rows must hold at least (x, y, w)")
        geom = plan_geometry(tn, nw_max, edge_cap, tower_ids, raw.device)
        if rows.shape[0] != geom.n_nodes:
            raise ValueError(f"raw has {rows.shape[0]} rows, towers hold {geom.n_nodes} nodes")
        thr = 0.0 if threshold is None else float(threshold)
        batch = DeviceTowerBatch(geom, ("positions", thr, float(divisor)), node_shape)
        if propagation is not None:
            batch.prop = _device_f32(propagation, "propagation").reshape(geom.n_nodes, 100)
        batch._fill(rows)
        if check:
            batch.check()
        return batch

    @staticmethod
    def from_dense_device(objects: torch.Tensor, sender_relations: torch.Tensor, receiver_relations: torch.Tensor,
                          propagation: Optional[torch.Tensor] = None, nw_max: Optional[int] = None,
                          check: bool = False) -> "DeviceTowerBatch":
        """`from_dense` for inputs that are already on the device (Networks.py:22-29): the relation
        matrices are scanned by one kernel (spwgnn_plan_device_dense, the semantics of
        spwgnn_dense_to_edges) into a capacity plan of N(N−1) slots per tower; nothing is copied to the
        host and nothing synchronises unless ``check=True`` (see `from_positions`). A non-None
        ``propagation`` is used as it is (an all-zero one is not detected)."""
        obj = _device_f32(objects, "objects")
        Rs = _device_f32(sender_relations, "sender_relations")
        Rr = _device_f32(receiver_relations, "receiver_relations")
        if obj.dim() != 3 or obj.shape[2] < 3:
            raise ValueError("objects must be (B, N, 3)")
        B, N = int(obj.shape[0]), int(obj.shape[1])
        E = N * (N - 1)
        if tuple(Rs.shape) != (B, N, E) or tuple(Rr.shape) != (B, N, E):
            raise ValueError(f"relation matrices must be (B, N, N(N-1)) = {(B, N, E)}; got {tuple(Rs.shape)}, "
                             f"{tuple(Rr.shape)}")
        geom = plan_geometry(_Uniform(B, N), nw_max, None, None, obj.device)
        batch = DeviceTowerBatch(geom, ("dense",), (B, N))
        batch.pos.zero_()
        batch.pos[:, :3] = obj.reshape(B * N, -1)[:, :3]
        if propagation is not None:
            batch.prop = _device_f32(propagation, "propagation").reshape(geom.n_nodes, 100)
        batch._fill((Rs, Rr))
        if check:
            batch.check()
        return batch

    def refill(self, source, check: bool = False) -> "TowerBatch":
        """Device-built batches only (`from_positions`, `from_dense_device`): fill the same device
        arrays again from new positions, or new (Rs, Rr) — in place, one launch, capturable."""
        raise _lib.SpwgnnError("refill needs a batch built on the device (TowerBatch.from_positions / from_dense_device)")

    # ------------------------------------------------------------------ C view
    def cstruct(self) -> _lib.BatchC:
        if self._cstruct is None:
            b = _lib.BatchC()
            b.n_towers, b.n_nodes = self.n_towers, self.n_nodes
            b.n_wtiles, b.n_eblocks, b.nw_max = self.n_wtiles, self.n_eblocks, self.nw_max
            b.flags = self.flags
            b.pos = self.pos.data_ptr()
            b.prop = self.prop.data_ptr() if self.prop is not None else None
            b.node_tower = self.node_tower.data_ptr()
            b.node_local = self.node_local.data_ptr()
            b.wtile = self.wtile.data_ptr()
            b.edge_src = self.edge_src.data_ptr()
            b.edge_dst = self.edge_dst.data_ptr()
            b.blk_csr = self.blk_csr.data_ptr()
            self._cstruct = b
        return self._cstruct

    def with_prop(self, prop: Optional[torch.Tensor]) -> "TowerBatch":
        """Same graph, different propagation input (device tensor (Nn, 100) or None)."""
        nb = TowerBatch(**{k: getattr(self, k) for k in self.__dataclass_fields__ if k != "_cstruct"})
        nb.prop = None if prop is None else prop.reshape(self.n_nodes, 100).to(self.device, torch.float32).contiguous()
        return nb


# ---------------------------------------------------------------------- plans built on the device
class _Uniform(tuple):
    """(B, N): B towers of N nodes each, without materialising the size array."""

    def __new__(cls, B: int, N: int):
        return super().__new__(cls, (int(B), int(N)))


def _device_f32(t, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise _lib.SpwgnnError(f"{what} must be a HIP device tensor; the device plan has no host path "
                               "(TowerBatch.from_dense / ragged take host data)")
    return t.detach().to(torch.float32).contiguous()


@dataclass
class PlanGeometry:
    """What a capacity plan fixes from the tower sizes and capacities alone (spwgnn_plan_size_cap /
    spwgnn_plan_fill_cap with zero edges): the host arrays, and — once `to` has uploaded them — the
    device tensors every device-built batch of this shape shares read-only."""
    n_towers: int
    n_nodes: int
    n_wtiles: int
    n_eblocks: int
    nw_max: int
    tower_nodes: np.ndarray     # (T,) int32
    tower_cap: np.ndarray       # (T,) int32 relations each tower's blocks are sized for
    default_cap: bool           # tower_cap is N(N−1) everywhere: no tower can exceed it
    wtile: np.ndarray           # (n_wtiles, 4) int32
    node_tower: np.ndarray      # (n_nodes,) int32
    node_local: np.ndarray      # (n_nodes,) int32
    wtile_tower: np.ndarray     # (n_wtiles,) int32 index of each wave-tile's first tower
    device: Optional[torch.device] = None
    dev: Optional[dict] = field(default=None, repr=False)   # name → device tensor

    def to(self, device) -> "PlanGeometry":
        if self.dev is None or self.device != torch.device(device):
            names = ["wtile", "node_tower", "node_local", "wtile_tower", "tower_cap"]
            self.dev = dict(zip(names, upload([getattr(self, n) for n in names], device)))
            self.device = torch.device(device)
        return self


def plan_geometry_host(tower_nodes, nw_max: Optional[int] = None, edge_cap=None, tower_ids=None) -> PlanGeometry:
    """The static arrays of a capacity plan, from the host planner given zero edges. ``tower_nodes``
    (T,) sizes; ``edge_cap`` scalar or (T,), default N(N−1) per tower. No device is touched."""
    tn = np.full(tower_nodes[0], tower_nodes[1], np.int32) if isinstance(tower_nodes, _Uniform) else \
        np.ascontiguousarray(tower_nodes, dtype=np.int32)
    T = len(tn)
    full = (tn.astype(np.int64) * (tn.astype(np.int64) - 1)).astype(np.int32)
    if edge_cap is None:
        cap = full
    else:
        cap = np.array(np.broadcast_to(np.asarray(edge_cap, np.int32), (T,)), dtype=np.int32)   # an own, writable copy
        if np.any(cap < 0):
            raise ValueError("edge_cap must be >= 0")
    empty = np.zeros(0, np.int32)
    plan = HostPlan.build(np.zeros((int(tn.sum()), 3), np.float32), tn, empty, empty, np.zeros(T, np.int32),
                          nw_max=nw_max, tower_ids=tower_ids, edge_cap=cap)
    wtile, node_tower, node_local = plan.arrays[3], plan.arrays[1], plan.arrays[2]
    starts = np.concatenate([[0], np.cumsum(tn)[:-1]]).astype(np.int64)
    wtile_tower = np.searchsorted(starts, wtile[:, 2].astype(np.int64)).astype(np.int32)
    return PlanGeometry(T, plan.n_nodes, plan.n_wtiles, plan.n_eblocks, plan.nw_max, tn, cap,
                        bool(np.all(cap >= full)), wtile, node_tower, node_local, wtile_tower)


_GEOMETRY_CACHE: dict = {}
_GEOMETRY_CACHE_MAX = 16


def plan_geometry(tower_nodes, nw_max: Optional[int] = None, edge_cap=None, tower_ids=None,
                  device="cuda") -> PlanGeometry:
    """`plan_geometry_host` uploaded to ``device``, cached per (tower sizes, nw_max, edge_cap,
    tower_ids, device): same-shape batches share the host planning, the upload and the arrays."""
    if isinstance(tower_nodes, _Uniform):
        tkey = ("uniform",) + tuple(tower_nodes)
    else:
        tower_nodes = np.ascontiguousarray(tower_nodes, dtype=np.int32)
        tkey = tower_nodes.tobytes()
    blob = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int64).tobytes()
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (tkey, None if nw_max is None else int(nw_max), blob(edge_cap), blob(tower_ids), str(dev))
    g = _GEOMETRY_CACHE.get(key)
    if g is None:
        g = plan_geometry_host(tower_nodes, nw_max, edge_cap, tower_ids).to(dev)
        while len(_GEOMETRY_CACHE) >= _GEOMETRY_CACHE_MAX:
            _GEOMETRY_CACHE.pop(next(iter(_GEOMETRY_CACHE)))
        _GEOMETRY_CACHE[key] = g
    return g


class DeviceTowerBatch(TowerBatch):
    """A TowerBatch whose edge arrays were filled on the device (TowerBatch.from_positions /
    from_dense_device). The geometry tensors are shared with every batch of the same shape; pos,
    edge_src, edge_dst, blk_csr, tower_edges_dev and the 4-byte ``status`` are this batch's own.

    There is no host edge list: ``src``, ``dst``, ``tower_edges``, ``edge_id`` and ``n_edges`` are
    fetched from the device on first access — a synchronising copy, which also raises `SpwgnnError`
    if the status word reports an error (see ``check``). The engine reads none of them."""

    def __init__(self, geom: PlanGeometry, source: tuple, node_shape):
        d, dev = geom.dev, geom.device
        self.geom, self.source = geom, source
        self.n_towers, self.n_nodes = geom.n_towers, geom.n_nodes
        self.tower_nodes = geom.tower_nodes
        self.n_wtiles, self.n_eblocks, self.nw_max = geom.n_wtiles, geom.n_eblocks, geom.nw_max
        self.device = dev
        self.pos = torch.empty(geom.n_nodes, 4, dtype=torch.float32, device=dev)
        self.prop = None
        self.node_tower, self.node_local, self.wtile = d["node_tower"], d["node_local"], d["wtile"]
        self.edge_src = torch.empty(geom.n_eblocks * 32, dtype=torch.int32, device=dev)
        self.edge_dst = torch.empty(geom.n_eblocks * 32, dtype=torch.int32, device=dev)
        self.blk_csr = torch.empty(geom.n_eblocks, 128, dtype=torch.uint8, device=dev)
        self.tower_edges_dev = torch.empty(geom.n_towers, dtype=torch.int32, device=dev)
        self.status = torch.empty(1, dtype=torch.int32, device=dev)
        self.node_shape = node_shape
        self.flags = 0
        self.node_perm = None
        self._cstruct = None
        self.generation = 0
        self._host = None   # (generation, src, dst, tower_edges, edge_id) once fetched

    def __repr__(self):
        return (f"DeviceTowerBatch(n_towers={self.n_towers}, n_nodes={self.n_nodes}, n_wtiles={self.n_wtiles}, "
                f"n_eblocks={self.n_eblocks}, nw_max={self.nw_max}, source={self.source[0]!r}, "
                f"generation={self.generation})")

    # ---- the one launch
    def _fill(self, source) -> None:
        g, d = self.geom, self.geom.dev
        p = _lib.PlanDeviceC()
        p.n_towers, p.n_nodes, p.n_wtiles, p.n_eblocks, p.nw_max = g.n_towers, g.n_nodes, g.n_wtiles, g.n_eblocks, g.nw_max
        p.wtile, p.node_local, p.wtile_tower = d["wtile"].data_ptr(), d["node_local"].data_ptr(), d["wtile_tower"].data_ptr()
        p.tower_cap = None if g.default_cap else d["tower_cap"].data_ptr()
        p.edge_src, p.edge_dst, p.blk_csr = self.edge_src.data_ptr(), self.edge_dst.data_ptr(), self.blk_csr.data_ptr()
        p.tower_edges, p.status = self.tower_edges_dev.data_ptr(), self.status.data_ptr()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.status.zero_()
        L = _lib.lib()
        if self.source[0] == "positions":
            rows = _device_f32(source, "raw")
            rows = rows.reshape(-1, rows.shape[-1])
            if rows.shape[0] != g.n_nodes or rows.shape[1] < 3:
                raise ValueError(f"raw must hold {g.n_nodes} rows of at least (x, y, w)")
            p.pos = self.pos.data_ptr()
            st = L.spwgnn_plan_device_positions(C.byref(p), rows.data_ptr(), int(rows.shape[1]), self.source[1],
                                                self.source[2], stream)
        else:
            Rs, Rr = (_device_f32(x, "relations") for x in source)
            B, N = self.node_shape
            if tuple(Rs.shape) != (B, N, N * (N - 1)) or tuple(Rr.shape) != tuple(Rs.shape):
                raise ValueError(f"relation matrices must be {(B, N, N * (N - 1))}")
            st = L.spwgnn_plan_device_dense(C.byref(p), Rs.data_ptr(), Rr.data_ptr(), B, N, stream)
        _lib.check(st, "spwgnn_plan_device_" + self.source[0])

    def refill(self, source, check: bool = False) -> "DeviceTowerBatch":
        """New positions (a `from_positions` batch: the ``raw`` tensor, same shape) or new relations (a
        `from_dense_device` batch: ``(Rs, Rr)``) into the SAME device arrays: one launch on the current
        stream, no synchronisation, capturable in a hipGraph (torch.cuda.graph) together with the
        forward. The generation counter moves on, so a forward stored on a `Workspace` before the
        refill no longer passes for this batch (`engine.Workspace.holds`): its backward is refused."""
        self.mark_refilled()
        self._fill(source)
        if check:
            self.check()
        return self

    def mark_refilled(self) -> None:
        """The device arrays hold a new relation set: `refill` calls this; call it yourself after
        replaying a captured graph that contains a refill (the replay does not pass through Python).
        Drops the fetched host fields and moves the generation on."""
        self.generation += 1
        self._host = None

    def check(self) -> "DeviceTowerBatch":
        """Read the 4-byte status word (a synchronising copy) and raise `SpwgnnError` if the fill
        reported an error: a malformed relation column, or a tower above its edge capacity."""
        st = int(self.status.item())
        if st:
            _lib.check(-st, "device plan (batch.status)")
        return self

    def _fetch(self):
        if self._host is None or self._host[0] != self.generation:
            self.check()
            es, ed = self.edge_src.cpu().numpy(), self.edge_dst.cpu().numpy()
            m = es >= 0
            eid = np.full(len(es), -1, np.int32)
            eid[m] = np.arange(int(m.sum()), dtype=np.int32)
            self._host = (self.generation, es[m], ed[m], self.tower_edges_dev.cpu().numpy(), eid)
        return self._host

    src = property(lambda self: self._fetch()[1], doc="(Ne,) global senders, fetched from the device (synchronises; see check)")
    dst = property(lambda self: self._fetch()[2], doc="(Ne,) global receivers, fetched from the device (synchronises)")
    tower_edges = property(lambda self: self._fetch()[3], doc="(T,) active relations per tower, fetched from the device")
    edge_id = property(lambda self: self._fetch()[4], doc="(n_eblocks*32,) edge index per slot or -1, fetched from the device")

    def edge_gates(self, values, fill: float = 0.0, device=None) -> torch.Tensor:
        """`TowerBatch.edge_gates` from the device's own edge arrays. The dense (B, N, N) [tower, sender,
        receiver] form (towers of one size) reads ``edge_src`` / ``edge_dst`` on the device: no host copy,
        no synchronisation, valid for the relation set the batch holds when the ops run. The 1-D form
        needs the host edge list (a synchronising fetch)."""
        v = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values))
        if v.dim() != 3:
            return TowerBatch.edge_gates(self, values, fill, device)
        tn = np.asarray(self.tower_nodes)
        if len(tn) == 0 or np.any(tn != tn[0]) or tuple(v.shape) != (len(tn), int(tn[0]), int(tn[0])):
            raise ValueError("the dense form needs towers of one size N and a (B, N, N) [tower, sender, receiver] "
                             f"tensor, got {tuple(v.shape)}")
        N = int(tn[0])
        v = v.to(device=self.device, dtype=torch.float32).reshape(-1)
        s, d = self.edge_src.long(), self.edge_dst.long()
        active = s >= 0
        got = v[torch.where(active, s * N + d % N, torch.zeros_like(s))]
        return torch.where(active, got, torch.full_like(got, float(fill))).contiguous()

    def with_prop(self, prop: Optional[torch.Tensor]) -> "DeviceTowerBatch":
        """Same graph and device arrays, different propagation input (no host field is touched)."""
        import copy
        nb = copy.copy(self)
        nb._cstruct = None
        nb.prop = None if prop is None else prop.reshape(self.n_nodes, 100).to(self.device, torch.float32).contiguous()
        return nb
