"""Multi-GPU layout of the hot path: corpus replicated per GPU, query batch sharded contiguously across
ranks, one all-gather of the fused top-k (BASELINE.json north_star).

Queries are independent units, so there is no data-path collective inside the retrieval itself; the only
exchange is the final gather of [B_local x k] (score, id, len) rows -- ~120 KB per rank at 1024 x 10, i.e. pure
latency on xGMI.  One process per GPU.  Three ways to run the gather, same result:

  "torch"   (default on GPUs) the library packs the rows (erh_pack_topk), `torch.distributed`
            all_gather_into_tensor (backend "nccl" = RCCL) moves ONE preallocated uint8 buffer, the library
            unpacks into preallocated global arrays (erh_unpack_topk): two tiny kernels + one collective, no
            per-step allocation, no torch.cat.
  "native"  erh_allgather_topk: pack + ncclAllGather + unpack inside the library on the caller's stream (its own
            RCCL communicator, bootstrapped by broadcasting erh_comm_unique_id through torch.distributed).
  "host"    CPU tensors / no engine: padded blocks through all_gather_into_tensor ("gloo" in the CPU tests).

The reference has no counterpart (single process, one query at a time: src/main.py:48-52).
"""
from __future__ import annotations

import os
import sys
from typing import Callable, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist


def shard_bounds(n_queries: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous shard [lo, hi) of rank `rank`; shards differ by at most one query."""
    base, rem = divmod(n_queries, world)
    lo = rank * base + min(rank, rem)
    hi = lo + base + (1 if rank < rem else 0)
    return lo, hi


def max_shard(n_queries: int, world: int) -> int:
    return (n_queries + world - 1) // world


def init_from_env(device_index: Optional[int] = None, backend: Optional[str] = None) -> Tuple[int, int]:
    """Initialise the default process group from RANK / WORLD_SIZE / MASTER_* (torchrun sets them).
    Returns (rank, world).  Single-process runs skip the group entirely.  `backend` (or ERH_DIST_BACKEND): "nccl" (= RCCL, the
    default on GPUs) or "gloo" -- the dry-run transport for several ranks on ONE GPU (RCCL does not share a device between
    ranks): QueryShards then stages the packed rows through the host, everything else is the same code."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world == 1:
        return 0, 1
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        use_gpu = torch.cuda.is_available()
        if use_gpu:
            if device_index is None:
                device_index = int(os.environ.get("LOCAL_RANK", "0"))
            torch.cuda.set_device(device_index)
        backend = backend or os.environ.get("ERH_DIST_BACKEND") or ("nccl" if use_gpu else "gloo")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world


def allgather_topk(ids: torch.Tensor, scores: torch.Tensor, lens: torch.Tensor, n_queries: int,
                   group=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """"host" gather: every rank's [B_local x k] fused top-k -> the global [n_queries x k] result, in query order.
    Shards are padded to max_shard rows so that all ranks contribute equal-sized blocks; the padding rows are
    dropped afterwards.  (GPU runs use QueryShards below, which packs in the library and allocates nothing.)"""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return ids[:n_queries], scores[:n_queries], lens[:n_queries]
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    m = max_shard(n_queries, world)
    lo, hi = shard_bounds(n_queries, rank, world)
    k = ids.shape[1]

    def pad(t, fill):
        if t.shape[0] == m:
            return t.contiguous()
        out = torch.full((m,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
        out[: hi - lo] = t[: hi - lo]
        return out

    p_ids, p_sc, p_ln = pad(ids, -1), pad(scores, 0), pad(lens, 0)
    nb_sc, nb_id, nb_ln = k * p_sc.element_size(), k * p_ids.element_size(), p_ln.element_size()
    packed = torch.cat([p_sc.view(torch.uint8).reshape(m, nb_sc), p_ids.view(torch.uint8).reshape(m, nb_id),
                        p_ln.reshape(m, 1).view(torch.uint8).reshape(m, nb_ln)], dim=1).contiguous()
    g = torch.empty((world * m, packed.shape[1]), dtype=torch.uint8, device=ids.device)
    dist.all_gather_into_tensor(g, packed, group=group)
    g_sc = g[:, :nb_sc].contiguous().view(scores.dtype).reshape(world * m, k)
    g_ids = g[:, nb_sc:nb_sc + nb_id].contiguous().view(ids.dtype).reshape(world * m, k)
    g_ln = g[:, nb_sc + nb_id:].contiguous().view(lens.dtype).reshape(world * m)
    if n_queries == world * m:
        return g_ids, g_sc, g_ln
    keep = torch.cat([torch.arange(r * m, r * m + (shard_bounds(n_queries, r, world)[1] - shard_bounds(n_queries, r, world)[0]),
                                   device=ids.device) for r in range(world)])
    return g_ids[keep], g_sc[keep], g_ln[keep]


class _RowGather:
    """The exchange both layouts share: every rank's block of packed rows (`send`) -> all blocks, rank after rank (`recv`).
    Returns the transport it used: "rccl", "gloo", "gloo-staged" (device rows through pinned host memory) or "local"."""

    def __init__(self):
        self._send_host = self._recv_host = None

    def all_gather(self, send: torch.Tensor, recv: torch.Tensor, world: int, group=None) -> str:
        if world == 1:
            recv.copy_(send)
            return "local"
        staged = send.is_cuda and dist.get_backend(group) == "gloo"
        if not staged:
            dist.all_gather_into_tensor(recv, send, group=group)
            return "rccl" if send.is_cuda else "gloo"
        # several ranks on ONE GPU (dry run of the multi-process path: RCCL does not share a device between ranks):
        # the packed rows cross the process boundary through pinned host memory; pack and unpack stay on the device
        if self._send_host is None or self._send_host.shape != send.shape:
            self._send_host = torch.empty(send.shape, dtype=send.dtype, pin_memory=True)
            self._recv_host = torch.empty(recv.shape, dtype=recv.dtype, pin_memory=True)
        self._send_host.copy_(send)                        # (synchronises: the pack kernel has finished)
        dist.all_gather_into_tensor(self._recv_host, self._send_host, group=group)
        recv.copy_(self._recv_host)
        return "gloo-staged"


class QueryShards:
    """One rank's view of a sharded global query batch: its contiguous shard and the gather of the results.

        sh = QueryShards(n_queries, rank, world, engine=eng)          # engine=None -> "host" gather (CPU tests)
        lo, hi = sh.bounds
        ids, sc, ln = sh.step(lambda lo, hi: eng.hybrid_topk(q[lo:hi], ..., device_out=True))

    `step` runs the local retrieval on [lo, hi) and returns the GLOBAL result on every rank.  bench.py --gpus N and
    the tests drive exactly this code."""

    def __init__(self, n_queries: int, rank: int, world: int, engine=None, mode: Optional[str] = None, group=None):
        self.n, self.rank, self.world, self.engine, self.group = int(n_queries), int(rank), int(world), engine, group
        self.bounds = shard_bounds(self.n, self.rank, self.world)
        self.m = max_shard(self.n, self.world)
        if mode is None:
            mode = os.environ.get("ERH_GATHER", "torch") if engine is not None else "host"
        if mode not in ("torch", "native", "host"):
            raise ValueError("gather mode must be torch, native or host")
        if mode != "host" and engine is None:
            raise ValueError("the packed gathers need the engine (the library packs and unpacks)")
        self.mode = mode
        self._k = None
        self._send = self._recv = self._out = None
        self._rows = _RowGather()
        self.fallback_reason = None
        self.transport = None                     # set by the first gather: "rccl", "gloo", "gloo-staged" (device rows through pinned host memory) or "local"
        if mode == "native" and world > 1:
            self._init_native()

    def _init_native(self):
        """Join the library's own RCCL communicator -- or, if any rank cannot (librccl not loadable, ncclCommInitRank
        failed or timed out), fall back to the "torch" gather on EVERY rank (the decision is an all-reduce, so no rank
        is left waiting inside a collective the others never enter)."""
        eng, rank, world, group = self.engine, self.rank, self.world, self.group
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")

        def all_ok(ok: bool) -> bool:
            t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
            return bool(int(t.item()))

        reason = None
        uid = None
        try:                                              # every rank probes its own librccl (cheap) before anyone blocks
            uid = eng.comm_unique_id()
        except Exception as exc:                          # noqa: BLE001 -- any failure means "not available here"
            reason = f"librccl not usable on rank {rank}: {exc}"
        if all_ok(reason is None):
            box = [uid if rank == 0 else None]
            dist.broadcast_object_list(box, src=0, group=group)
            try:
                eng.comm_init(rank, world, box[0])
            except Exception as exc:                      # noqa: BLE001
                reason = f"erh_comm_init failed on rank {rank}: {exc}"
            if not all_ok(reason is None):
                reason = reason or "erh_comm_init failed on another rank"
                try:
                    eng.comm_destroy()                    # (a rank whose own init timed out: the library reaps the late communicator)
                except Exception:                         # noqa: BLE001
                    pass
        else:
            reason = reason or "librccl not usable on another rank"
        if reason is not None:
            self.mode, self.fallback_reason = "torch", reason
            print(f"[easyrag_amd.dist] rank {rank}: native gather unavailable, using torch.distributed ({reason})",
                  file=sys.stderr, flush=True)

    def _buffers(self, k: int, device):
        if self._k != k:
            row = self.engine.topk_row_bytes(k)
            self._send = torch.empty((self.m, row), dtype=torch.uint8, device=device)
            self._recv = torch.empty((self.m * self.world, row), dtype=torch.uint8, device=device)
            self._out = (torch.empty((self.n, k), dtype=torch.int32, device=device),
                         torch.empty((self.n, k), dtype=torch.float64, device=device),
                         torch.empty((self.n,), dtype=torch.int32, device=device))
            self._k = k
        return self._send, self._recv, self._out

    def gather(self, ids, sc, ln, check: bool = True):
        """All-gather this rank's [B_local x k] result.  `check` (default): erh_dense_check first.  Since round 5 a dense / fused call
        with device outputs enqueues only the COUNT of the queries its candidate budgets could not certify; EVERY answering round of
        the exhaustive path (and the re-run of the fusion over the corrected lists, and of a routed call's flagged groups) runs inside
        erh_dense_check, so rows must not leave the rank before it has run.  check=False is for callers that have called
        `engine.dense_check()` themselves since the last dense / fused call -- skipping it altogether hands out uncertified lists."""
        lo, hi = self.bounds
        if ids.shape[0] != hi - lo:
            raise ValueError(f"rank {self.rank} must contribute its shard of {hi - lo} queries, got {ids.shape[0]}")
        if self.mode == "host":
            return allgather_topk(ids, sc, ln, self.n, self.group)
        if check:
            self.engine.dense_check()                      # (returns at once when the last call had no dense route)
        k = int(ids.shape[1])
        send, recv, out = self._buffers(k, ids.device)
        if self.mode == "native":
            return self.engine.allgather_topk(ids, sc, ln, self.n, out=out)
        self.engine.pack_topk(ids, sc, ln, send)
        self.transport = self._rows.all_gather(send, recv, self.world, self.group)
        self.engine.unpack_topk(recv, self.n, self.world, k, out)
        return out

    def step(self, run_local: Callable[[int, int], Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]):
        lo, hi = self.bounds
        return self.gather(*run_local(lo, hi))


# ---- the other layout: the CORPUS cut across ranks -----------------------------------------------------------------------------
#
# Rank r holds the contiguous rows [lo_r, hi_r) of the corpus (chunk matrix, postings, class column) and answers ALL queries of a
# call on them; the ranks all-gather their packed lists and every rank merges (dense, BM25) or merges and fuses (hybrid) on its own
# device (erh_shard_merge_topk / erh_shard_rrf).  What it buys that replicas cannot: a single query streams N / world rows per GPU,
# and the corpus may be `world` times what one card holds.  The result equals the unsharded call bit for bit:
# scores depend on (query, document) only, the slices' BM25 payloads are computed with the GLOBAL idf / avgdl
# (index.slice_bm25_index), and canonical lists of contiguous slices merge canonically.  The reference has no counterpart.

def corpus_shard_bounds(n_docs: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous slice [lo, hi) of the corpus held by rank `rank`; slices differ by at most one row."""
    return shard_bounds(n_docs, rank, world)


def _pack_rows_host(ids, sc, ln) -> torch.Tensor:
    """erh_pack_topk's row format [k x f64 | k x i32 | i32 len | pad to 8] from host arrays ("host" mode: no engine)."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    sc = np.ascontiguousarray(sc, dtype=np.float64)
    ln = np.ascontiguousarray(ln, dtype=np.int32)
    B, k = ids.shape
    row = (12 * k + 4 + 7) // 8 * 8
    out = np.zeros((B, row), np.uint8)
    out[:, :8 * k] = sc.view(np.uint8).reshape(B, 8 * k)
    out[:, 8 * k:12 * k] = ids.view(np.uint8).reshape(B, 4 * k)
    out[:, 12 * k:12 * k + 4] = ln.reshape(B, 1).view(np.uint8)
    return torch.from_numpy(out)


def _merge_rows_host(recv: np.ndarray, B: int, world: int, k: int, id_base: np.ndarray):
    """What erh_shard_merge_topk computes, on the host ("host" mode without an engine: the CPU dry run of the exchange)."""
    recv = np.ascontiguousarray(recv).reshape(world, B, -1)
    sc = np.ascontiguousarray(recv[:, :, :8 * k]).view(np.float64).reshape(world, B, k)
    ids = np.ascontiguousarray(recv[:, :, 8 * k:12 * k]).view(np.int32).reshape(world, B, k).astype(np.int64)
    ln = np.ascontiguousarray(recv[:, :, 12 * k:12 * k + 4]).view(np.int32).reshape(world, B)
    o_ids = np.full((B, k), -1, np.int32)
    o_sc = np.zeros((B, k), np.float64)
    o_ln = np.zeros(B, np.int32)
    for q in range(B):
        g = np.concatenate([ids[r, q, :ln[r, q]] + int(id_base[r]) for r in range(world)])
        s = np.concatenate([sc[r, q, :ln[r, q]] for r in range(world)])
        order = np.lexsort((g, -s))[:k]
        o_ln[q] = order.size
        o_ids[q, :order.size] = g[order]
        o_sc[q, :order.size] = s[order]
    return torch.from_numpy(o_ids), torch.from_numpy(o_sc), torch.from_numpy(o_ln)


class CorpusShards:
    """One rank's view of a corpus cut into contiguous slices -- the sibling of QueryShards.

        cs = CorpusShards(n_docs, rank, world, engine=eng)                 # eng holds rows [lo, hi) only
        cs.load(x, bm25_index, content_id, dir_id)                         # full arrays in; uploads this rank's part
        ids, sc, ln = cs.hybrid_topk(q, q_indptr, q_tok, k_dense=288, k_sparse=192, K=60, topk=256)
        ids, sc, ln = cs.dense_topk(q, k);  cs.bm25_topk(q_indptr, q_tok, k)

    Every call returns the GLOBAL result (global document ids) on every rank, as device tensors.  Transports: "torch" (default;
    RCCL, or gloo staged through pinned host memory when several ranks share one GPU) and "host"; "native" -- erh_allgather_topk
    unpacks into query-shard order, which is not this layout -- runs as "torch" on every rank, the reason in `fallback_reason`.
    engine=None ("host" only) is the CPU dry run of the exchange: `merge_topk` over canned lists, merged on the host.

    `CorpusShards.local(n_docs, engines)` is the one-process form: one handle per slice, on one device or several, lists copied
    device to device, merged on the first handle's device.  Set filters (dense_topk_sets) and the retriever classes are not
    available over a sharded corpus."""

    def __init__(self, n_docs: int, rank: int, world: int, engine=None, mode: Optional[str] = None, group=None,
                 _engines=None):
        self.n_docs, self.world, self.group = int(n_docs), int(world), group
        if self.world < 1 or self.n_docs < 1:
            raise ValueError("n_docs and world must be positive")
        if self.world > self.n_docs:
            raise ValueError(f"{self.world} slices of a corpus of {self.n_docs} rows: a slice would be empty")
        self.local_form = _engines is not None
        self.fallback_reason = None
        self.transport = None
        if self.local_form:
            if len(_engines) != self.world:
                raise ValueError("the one-process form needs one engine per slice")
            self.engines, self.ranks, self.rank, self.mode = list(_engines), list(range(self.world)), None, "local"
        else:
            self.rank = int(rank)
            if not 0 <= self.rank < self.world:
                raise ValueError("rank out of range")
            if mode is None:
                mode = os.environ.get("ERH_GATHER", "torch") if engine is not None else "host"
            if mode not in ("torch", "native", "host"):
                raise ValueError("gather mode must be torch, native or host")
            if mode != "host" and engine is None:
                raise ValueError("the packed gathers need the engine (the library packs and merges)")
            if mode == "native":                   # the same decision on every rank, so nobody waits in a collective alone
                mode = "torch"
                self.fallback_reason = ("erh_allgather_topk unpacks into query-shard order; the corpus-sharded layout gathers "
                                        "raw rows through torch.distributed")
            self.mode = mode
            self.engines, self.ranks = ([engine] if engine is not None else []), [self.rank]
        self.engine = self.engines[0] if self.engines else None          # the handle that merges
        self.id_base = np.array([corpus_shard_bounds(self.n_docs, r, self.world)[0] for r in range(self.world)], np.int32)
        self.bounds = corpus_shard_bounds(self.n_docs, self.rank, self.world) if self.rank is not None else (0, self.n_docs)
        self._rows = _RowGather()
        self._bufs = {}

    @classmethod
    def local(cls, n_docs: int, engines):
        """One process drives every slice: engines[r] holds slice r."""
        return cls(n_docs, 0, len(engines), _engines=engines)

    # -- corpus state ----------------------------------------------------------------------------------------------
    def load(self, x=None, bm25_index=None, content_id=None, dir_id=None, payload_on_device: bool = False,
             normalize: bool = False, slot: Optional[int] = None):
        """Full arrays in: every engine of this object gets ITS rows of the chunk matrix `x`, its slice of the BM25 index (global
        idf / avgdl) and of the class column `dir_id`; the GLOBAL `content_id` goes to the merging handle."""
        from .index import slice_bm25_index
        for eng, r in zip(self.engines, self.ranks):
            lo, hi = corpus_shard_bounds(self.n_docs, r, self.world)
            with self._on(eng):
                if x is not None:
                    if int(x.shape[0]) != self.n_docs:
                        raise ValueError("x must hold every row of the corpus")
                    eng.set_dense(x[lo:hi], normalize=normalize)
                if bm25_index is not None:
                    if bm25_index.n_docs != self.n_docs:
                        raise ValueError("the BM25 index must cover the whole corpus")
                    eng.set_bm25(slice_bm25_index(bm25_index, lo, hi), payload_on_device=payload_on_device, slot=slot)
                if dir_id is not None:
                    eng.set_doc_meta(hi - lo, None, np.asarray(dir_id)[lo:hi])
        if content_id is not None:
            if len(content_id) != self.n_docs:
                raise ValueError("content_id must have one entry per document of the whole corpus")
            with self._on(self.engine):
                self.engine.set_shard_content(content_id)

    # -- helpers ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _on(eng):
        return torch.cuda.device(eng.device)

    def _buffers(self, tag: str, B: int, k: int):
        """Per (route, B, k): one send block per engine on its device, the receive block on the merging device."""
        key = (tag, B, k)
        if key not in self._bufs:
            row = self.engine.topk_row_bytes(k)
            send = [torch.empty((B, row), dtype=torch.uint8, device=torch.device("cuda", e.device)) for e in self.engines]
            recv = torch.empty((self.world, B, row), dtype=torch.uint8, device=torch.device("cuda", self.engine.device))
            self._bufs[key] = (send, recv)
        return self._bufs[key]

    def _exchange(self, send, recv):
        if self.local_form:
            for r, s in enumerate(send):
                recv[r].copy_(s)                       # device to device (the same device, or a peer)
            self.transport = "device-copy"
        else:
            self.transport = self._rows.all_gather(send[0], recv.view(self.world * recv.shape[1], recv.shape[2]),
                                                   self.world, self.group)

    def _need_engine(self):
        if self.engine is None:
            raise RuntimeError("this CorpusShards has no engine (host dry run): only merge_topk is available")

    @staticmethod
    def _q_for(eng, q):
        if isinstance(q, torch.Tensor) and q.is_cuda and q.device.index != eng.device:
            return q.to(torch.device("cuda", eng.device))
        return q

    def _run(self, routes, B):
        """routes: [(tag, k, fn(engine) -> device lists)].  Every engine answers every route on its slice, certifies the dense
        lists (dense_check: a stream sync alone is not enough for them) and packs; then one exchange per route."""
        bufs = [self._buffers(tag, B, k) for tag, k, _ in routes]
        for j, eng in enumerate(self.engines):
            with self._on(eng):
                lists = [fn(eng) for _, _, fn in routes]
                eng.dense_check()                      # (returns at once when no route was dense)
                for (send, _), (ids, sc, ln) in zip(bufs, lists):
                    eng.pack_topk(ids, sc, ln, send[j])
        with self._on(self.engine):
            for send, recv in bufs:
                self._exchange(send, recv)
        return [recv for _, recv in bufs]

    # -- queries ---------------------------------------------------------------------------------------------------
    def merge_topk(self, ids, sc, ln):
        """This rank's lists for ALL queries ([B x k], local ids) -> the global lists on every rank.  The engines' own results go
        through dense_topk / bm25_topk / hybrid_topk; this entry serves callers that hold lists already and the host dry run."""
        if self.local_form:
            raise RuntimeError("merge_topk is the per-rank entry; the one-process form runs its slices itself")
        B, k = int(ids.shape[0]), int(ids.shape[1])
        if self.engine is None:
            send = _pack_rows_host(ids, sc, ln)
            recv = torch.empty((self.world * B, send.shape[1]), dtype=torch.uint8)
            self.transport = self._rows.all_gather(send, recv, self.world, self.group)
            return _merge_rows_host(recv.numpy(), B, self.world, k, self.id_base)
        recv, = self._run([("merge", k, lambda eng: (ids, sc, ln))], B)
        with self._on(self.engine):
            return self.engine.shard_merge_topk(recv, B, self.world, k, self.id_base)

    def dense_topk(self, q, k: int, filter_dir=None, mode: int = 0, normalize_q: bool = False):
        self._need_engine()
        B = int(q.shape[0]) if getattr(q, "ndim", 2) == 2 else 1
        recv, = self._run([("dense", int(k), lambda eng: eng.dense_topk(self._q_for(eng, q), k, filter_dir=filter_dir, mode=mode,
                                                                      normalize_q=normalize_q, device_out=True))], B)
        with self._on(self.engine):
            return self.engine.shard_merge_topk(recv, B, self.world, int(k), self.id_base)

    def bm25_topk(self, q_indptr, q_tok, k: int, filter_dir=None, slot: Optional[int] = None):
        self._need_engine()
        B = int(len(q_indptr)) - 1
        recv, = self._run([("bm25", int(k), lambda eng: eng.bm25_topk(q_indptr, q_tok, k, filter_dir=filter_dir, device_out=True,
                                                                    slot=slot))], B)
        with self._on(self.engine):
            return self.engine.shard_merge_topk(recv, B, self.world, int(k), self.id_base)

    def hybrid_topk(self, q, q_indptr, q_tok, k_dense: int = 288, k_sparse: int = 192, K: int = 60, topk: int = 256,
                    filter_dir=None, normalize_q: bool = False, slot: Optional[int] = None, filter_dense="same"):
        """RetrievalEngine.hybrid_topk over the sharded corpus: filter_dir restricts the sparse route, filter_dense (default: the
        same column) the dense one; both go to every slice's class column unchanged (class ids are global)."""
        self._need_engine()
        B = int(len(q_indptr)) - 1
        fdn = filter_dir if isinstance(filter_dense, str) else filter_dense
        r_sp, r_dn = self._run([
            ("sparse", int(k_sparse), lambda eng: eng.bm25_topk(q_indptr, q_tok, k_sparse, filter_dir=filter_dir, device_out=True,
                                                                slot=slot)),
            ("dense", int(k_dense), lambda eng: eng.dense_topk(self._q_for(eng, q), k_dense, filter_dir=fdn,
                                                               normalize_q=normalize_q, device_out=True))], B)
        with self._on(self.engine):
            return self.engine.shard_rrf(r_sp, int(k_sparse), r_dn, int(k_dense), B, self.world, self.id_base, K=K, topk=topk)
