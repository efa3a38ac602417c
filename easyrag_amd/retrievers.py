"""Drop-in retrievers with the reference's class names, constructor kwargs, methods and return
conventions, backed by libeasyrag_hip.so (MI355X).  Mirrors
/root/reference/src/easyrag/custom/retrievers.py:

  QdrantRetriever(vector_store, embed_model, similarity_top_k=2, filters=None)      ref :23-69
  tokenize_and_remove_stopwords(tokenizer, text, stopwords)                          ref :72-76
  BM25Retriever(nodes, tokenizer, similarity_top_k, ..., stopwords, embed_type, bm25_type)
      .get_scores(query, docs=None) / .from_defaults(...) / .filter(scores) / ._retrieve   ref :80-220
  HybridRetriever(dense_retriever, sparse_retriever, retrieval_type=1, topk=256)
      .fusion(lists, topk) / .reciprocal_rank_fusion(lists, K, topk) / ._aretrieve     ref :223-305

What differs, deliberately: nodes are addressed by their integer position in the caller's node list
(the pipeline keeps the same map, pipeline.py:221-223); the Qdrant collection is replaced by
HipVectorStore (the fp16 chunk matrix resident in HBM); equal scores are ordered by node index
(numpy's argsort()[::-1] tie order is implementation-defined); and every retriever also offers a
batched entry point (retrieve_batch) because the GPU path is built for batches.  Scores, cut-offs,
filters, fusion keys and list order follow the reference -- including HybridRetriever's two faces:
`aretrieve` (what the pipeline calls) selects the route and fuses with RRF, `retrieve` is the reference's
unmaintained sync path (sparse + dense concatenated, de-duplicated by node_id, no fusion, no filter push-down).

Engine sharing: retrievers built over the same node list may share one RetrievalEngine (one GPU replica of
the corpus): the vector store holds the chunk matrix, every BM25Retriever takes its own BM25 index slot of the
engine (4 per engine), and the node bookkeeping (content ids, filter classes) lives on the engine.  Passing an
engine that already serves a DIFFERENT node list raises.

No retrieval arithmetic happens in this file except BM25Retriever.filter(scores), which the reference
exposes as a host-side helper over a caller-supplied score vector; _retrieve does not use it.
"""
from __future__ import annotations

import asyncio
import logging
import threading
from typing import Any, Callable, Dict, Hashable, List, Optional, Sequence

import numpy as np

from . import _lib
from .engine import RetrievalEngine, queries_to_csr
from .index import BM25Index, build_bm25_index, vocab_ids
from .schema import NodeWithScore, QueryBundle, TextNode

logger = logging.getLogger(__name__)

DEFAULT_SIMILARITY_TOP_K = 2   # llama_index.core.constants.DEFAULT_SIMILARITY_TOP_K
BM25_DEVICE_MAX_K = 1024       # erh_bm25_topk / erh_hybrid_topk: k_sparse <= 1024
DENSE_MAX_K = 768              # erh_dense_topk / erh_hybrid_topk: k_dense <= 768
FUSE_MAX_ITEMS = 2048          # erh_rrf / erh_fusion / erh_hybrid_topk: items of both lists together


# ---------------------------------------------------------------------------------------------------
# text variants and tokenisation (host side, as in the reference)
def _join_overlapping(head: str, tail: str) -> str:
    """`head` followed by `tail` with the longest suffix-of-head == prefix-of-tail written once (ref ingestion.py:20-31)."""
    keep = 0
    for i in range(1, min(len(head), len(tail)) + 1):
        if head[-i:] == tail[:i]:
            keep = i
    return head + tail[keep:]


def _previous_node_id(node):
    """node_id of the PREVIOUS relationship of a NodeWithScore's node (llama_index keys the dict by the
    NodeRelationship enum, whose value is the string "2"; the stand-in nodes may use either or the name)."""
    rel = node.node.relationships
    try:
        from llama_index.core.schema import NodeRelationship  # type: ignore
        return rel[NodeRelationship.PREVIOUS].node_id
    except ImportError:
        for key in ("PREVIOUS", "2", 2):
            if key in rel:
                return rel[key].node_id
        raise KeyError("PREVIOUS")


def _table_with_header(node, text: str, nodes, nodeid2idx) -> str:
    """embed_type 6 (ref ingestion.py:36-57): a chunk that looks like the body of a markdown table (>= 5 '|', no '---'
    rule) is joined with up to three preceding chunks until one of them carries the table's header rule; the result is the
    header line + everything from the rule on.  Without a rule within three chunks the text stays as it was."""
    if text.count("|") < 5 or text.count("---") != 0:
        return text
    cur, found = text, False
    for _ in range(3):
        # (the reference never advances past the first PREVIOUS link: it re-reads node.node's relationship on every
        # turn, so the same predecessor is merged up to three times -- kept, the merge is idempotent after the first)
        pre_text = nodes[nodeid2idx[_previous_node_id(node)]].text
        cur = _join_overlapping(pre_text, cur)
        if pre_text.count("---") >= 2:
            found = True
            break
    if not found:
        return text
    at = cur.index("---")
    return cur[:at].strip().split("\n")[-1] + cur[at:]


def get_node_content(node, embed_type: int = 0, nodes=None, nodeid2idx=None) -> str:
    """Text fed to a route, by embed_type (ref: src/easyrag/pipeline/ingestion.py:34-76).
    0 raw text; 1 '###\\n<file_path>\\n\\n<text>'; 2 same with know_path; 3 image captions expanded;
    4 file_path only; 5 know_path only; 6 = 3 after the table-header merge over the PREVIOUS relationship, which
    needs a NodeWithScore plus the pipeline's `nodes` / `nodeid2idx` (as the reference does: with a bare TextNode a
    table-like chunk raises AttributeError there and here)."""
    text = node.get_content()
    meta = node.metadata
    if embed_type == 6:
        text = _table_with_header(node, text, nodes, nodeid2idx)
    if embed_type == 1 and "file_path" in meta:
        return "###\n" + meta["file_path"] + "\n\n" + text
    if embed_type == 2 and "know_path" in meta:
        return "###\n" + meta["know_path"] + "\n\n" + text
    if embed_type in (3, 6):
        for img in meta.get("imgobjs") or []:
            text = text.replace(f"{img['cap']} {img['title']}\n", f"{img['cap']}.{img['title']}:{img['content']}\n")
        return text
    if embed_type == 4:
        return meta.get("file_path", "")
    if embed_type == 5:
        return meta.get("know_path", "")
    return text


def tokenize_and_remove_stopwords(tokenizer, text, stopwords):
    """``tokenizer.cut(text)`` minus stop-words and single spaces (ref retrievers.py:72-76)."""
    return [w for w in tokenizer.cut(text) if w not in stopwords and w != " "]


def _unit_f16(v, slab_rows: int = 65536) -> np.ndarray:
    """L2-normalise rows in float64, round once to float16: the query / chunk representation the kernels score.
    (Qdrant normalises both sides for Distance.COSINE; doing it here pins the fp16 rounding on the host.)
    Rows go through float64 in slabs, so a 1M x 1024 matrix needs ~0.5 GB of temporaries, not 24."""
    v = np.asarray(v)
    if v.ndim == 1:
        v = v[None, :]
    out = np.empty(v.shape, np.float16)
    for r0 in range(0, v.shape[0], slab_rows):
        v64 = v[r0:r0 + slab_rows].astype(np.float32).astype(np.float64)
        n = np.sqrt(np.sum(v64 * v64, axis=-1, keepdims=True))
        n = np.where(n != 0.0, n, 1e-12)
        out[r0:r0 + slab_rows] = (v64 / n).astype(np.float16)
    return out


def _as_bundle(q) -> QueryBundle:
    return q if isinstance(q, QueryBundle) else QueryBundle(query_str=str(q))


class _TooManyClasses(ValueError):
    """More distinct value tuples than the int16 class column can number.  The sparse route reports it; the dense route serves such a
    filter through explicit row lists instead (HipVectorStore.query_batch)."""


class _MetaClasses:
    """Per-document class ids for an equality filter over a fixed set of metadata keys."""

    def __init__(self, nodes, keys: Sequence[str]):
        self.keys = tuple(keys)
        self.values: Dict[tuple, int] = {}
        ids = np.empty(len(nodes), np.int16)
        for i, n in enumerate(nodes):
            v = tuple(n.metadata.get(k) for k in self.keys)
            j = self.values.get(v)
            if j is None:
                j = len(self.values)
                if j >= 32000:
                    raise _TooManyClasses("too many distinct filter values")
                self.values[v] = j
            ids[i] = j
        self.ids = ids

    def class_of(self, filter_dict: Dict[str, Any]) -> int:
        v = tuple(filter_dict.get(k) for k in self.keys)
        return self.values.get(v, 32767)          # 32767 matches no document


# ---------------------------------------------------------------------------------------------------
# Qdrant payload filters beyond the pipeline's equality shape.  The reference's QdrantRetriever hands `filters` to Qdrant unchanged
# (ref retrievers.py:44-47), so any Qdrant filter works there.  Here a filter is compiled (duck typing on Qdrant's attribute names:
# qdrant_client's models and stand-ins with the same fields both work) into a hashable tree, evaluated on the host once per distinct
# value tuple of the class column over the keys it mentions, and reaches the device as the SET of classes a query may see.  Values
# compare as Python does (1 == 1.0 == True: the class column keys its classes by them), and a metadata value None counts as an absent
# key (the class column does not tell the two apart either).  Grammar (restated from Qdrant's documentation,
# unpinned like the rest of the third-party surface): Filter(must, should, must_not) with nesting, FieldCondition(key, match=MatchValue
# / MatchAny / MatchExcept) and FieldCondition(key, range=Range(gt, gte, lt, lte)); anything else raises TypeError.
_FILTER_VALUE_TYPES = (str, int, float, bool)


def _clause(v) -> list:
    if v is None:
        return []
    return list(v) if isinstance(v, (list, tuple)) else [v]


def _value(v, where: str):
    if isinstance(v, np.generic):
        v = v.item()
    if not isinstance(v, _FILTER_VALUE_TYPES):
        raise TypeError(f"unsupported filter value {v!r} in {where}")
    return v


def _bound(v, where: str):
    if v is None:
        return None
    if isinstance(v, np.generic):
        v = v.item()
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"unsupported Range bound {v!r} in {where} (numbers only)")
    return v


def _compile_condition(c, keys: set):
    """One condition -> a hashable tree node; `keys` collects the metadata keys it mentions."""
    name = type(c).__name__
    if hasattr(c, "has_id"):                                       # HasIdCondition: no payload condition (see _lift_id_conditions)
        raise TypeError(f"unsupported place for {name}: a HasIdCondition is served directly inside the top-level must (a rows= list) or "
                        f"must_not (an exclusion) of a retriever's filter, nowhere else: {c!r}")
    name = type(c).__name__
    if hasattr(c, "key"):                                          # FieldCondition
        key = c.key
        if not isinstance(key, str) or "." in key or "[" in key:
            raise TypeError(f"unsupported FieldCondition key {key!r} (nested / array key paths)")
        for attr in ("geo_bounding_box", "geo_radius", "geo_polygon", "values_count", "is_empty", "is_null"):
            if getattr(c, attr, None) is not None:
                raise TypeError(f"unsupported FieldCondition element {attr} on key {key!r}")
        match, rng = getattr(c, "match", None), getattr(c, "range", None)
        if (match is None) == (rng is None):
            raise TypeError(f"unsupported FieldCondition on key {key!r}: exactly one of match / range is supported")
        keys.add(key)
        if rng is not None:
            where = f"Range on {key!r}"
            for attr in ("gt", "gte", "lt", "lte"):
                if not hasattr(rng, attr):
                    raise TypeError(f"unsupported range object {type(rng).__name__} on key {key!r}")
            return ("range", key, _bound(rng.gt, where), _bound(rng.gte, where), _bound(rng.lt, where), _bound(rng.lte, where))
        mname = type(match).__name__
        if hasattr(match, "any"):                                  # MatchAny
            return ("any", key, tuple(sorted({_value(v, f"{mname} on {key!r}") for v in _clause(match.any)}, key=repr)))
        exc = getattr(match, "except_", None)
        if exc is None:
            exc = getattr(match, "except", None)
        if exc is not None or hasattr(match, "except_"):           # MatchExcept (attribute `except_`, alias `except`)
            return ("except", key, tuple(sorted({_value(v, f"{mname} on {key!r}") for v in _clause(exc)}, key=repr)))
        if hasattr(match, "value") and not hasattr(match, "text"):  # MatchValue
            return ("eq", key, _value(match.value, f"{mname} on {key!r}"))
        raise TypeError(f"unsupported match {mname} on key {key!r} (MatchValue / MatchAny / MatchExcept only)")
    if any(hasattr(c, a) for a in ("must", "should", "must_not")):  # Filter (nesting)
        if getattr(c, "min_should", None) is not None:
            raise TypeError("unsupported Filter element min_should")
        return ("filter", tuple(_compile_condition(x, keys) for x in _clause(getattr(c, "must", None))),
                tuple(_compile_condition(x, keys) for x in _clause(getattr(c, "should", None))),
                tuple(_compile_condition(x, keys) for x in _clause(getattr(c, "must_not", None))))
    raise TypeError(f"unsupported filter condition {name}: {c!r}")


def _holds(node, meta: Dict[str, Any]) -> bool:
    """Evaluate a compiled node on one row's metadata ({key: value}, absent keys missing)."""
    op = node[0]
    if op == "filter":
        _, must, should, must_not = node
        return (all(_holds(x, meta) for x in must) and (not should or any(_holds(x, meta) for x in should))
                and not any(_holds(x, meta) for x in must_not))
    if op == "both":                                               # a filter_dict AND a compiled filter (_both): the class column's
        return all(meta.get(k) == v for k, v in node[1]) and _holds(node[2], meta)   # equality (an absent key equals None), then the tree
    key = node[1]
    if key not in meta:
        return False                                               # a row without the key fails every condition on it
    v = meta[key]
    if op == "range":
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            return False
        gt, gte, lt, lte = node[2:]
        return ((gt is None or v > gt) and (gte is None or v >= gte) and (lt is None or v < lt) and (lte is None or v <= lte))
    if op == "eq":
        return v == node[2]
    hit = any(v == w for w in node[2])
    return hit if op == "any" else not hit


class _SetFilter:
    """A compiled filter that is not the equality shape: its tree and the metadata keys it mentions (its key set)."""

    __slots__ = ("node", "keys")

    def __init__(self, node, keys: Sequence[str]):
        self.node = node
        self.keys = tuple(sorted(keys))

    def __iter__(self):                        # iterates like a dict's keys: _by_key_set / key-set checks treat both alike
        return iter(self.keys)

    def __bool__(self):
        return True


_MATCH_NOTHING = _SetFilter(("filter", (), (), (("filter", (), (), ()),)), ())   # must_not=[empty Filter]: no row


def _filter_spec(filters):
    """None / {key: value} dict / Qdrant-style Filter -> None (unfiltered), a dict (the equality shape: exactly today's class column),
    or a _SetFilter.  Unsupported elements raise TypeError here, before any engine call."""
    if filters is None:
        return None
    if isinstance(filters, dict):
        return dict(filters) or None
    keys: set = set()
    node = _compile_condition(filters, keys)
    if node[0] != "filter":
        raise TypeError(f"unsupported filter object: {filters!r} (a Filter is expected at the top level)")
    _, must, should, must_not = node
    if not must and not should and not must_not:
        return None                                                # an empty Filter matches every row
    if (must and not should and not must_not and all(x[0] == "eq" for x in must)
            and len({x[1] for x in must}) == len(must)):
        return {x[1]: x[2] for x in must}                          # Filter(must=[MatchValue, ...]): the pipeline's shape
    if not keys:                                                   # nested empty filters only: a constant
        return None if _holds(node, {}) else _MATCH_NOTHING
    return _SetFilter(node, keys)


def _both(d: Optional[Dict[str, Any]], f):
    """The sparse route's two filters of one query as ONE spec: the rows that pass the filter_dict `d` AND the compiled `filters` entry `f`
    (None, a dict or a _SetFilter).  Two dicts merge (contradicting values match nothing); a dict beside a set filter becomes a set filter
    over the union of their keys, so that its class set is the intersection of the two filters' class sets in the column over those keys."""
    if not d:
        return f
    if not f:
        return d
    if isinstance(f, dict):
        if any(k in d and d[k] != v for k, v in f.items()):
            return _MATCH_NOTHING
        return {**d, **f}
    return _SetFilter(("both", tuple(sorted(d.items(), key=repr)), f.node), set(d) | set(f.keys))


def _filter_to_dict(filters) -> Optional[Dict[str, Any]]:
    """The equality shape only (None, a {key: value} dict, Filter(must=[FieldCondition(key, match=MatchValue(value))]) as
    build_qdrant_filters returns it, ref ingestion.py:207-216); other filters raise TypeError.  The retrievers use _filter_spec."""
    spec = _filter_spec(filters)
    if isinstance(spec, _SetFilter):
        raise TypeError(f"not an equality filter: {filters!r}")
    return spec


def _spec_cache() -> Callable[[Any], Any]:
    """_filter_spec with one compilation per distinct filter object of a batch (a per-query list repeats the same few)."""
    seen: Dict[int, tuple] = {}

    def spec(v):
        hit = seen.get(id(v))
        if hit is None:
            hit = seen[id(v)] = (v, _filter_spec(v))     # (v is held, so its id stays its own for the batch)
        return hit[1]
    return spec


def _spec_keys(spec) -> tuple:
    return tuple(sorted(spec)) if spec else ()


class _FilteredCorpus:
    """Shared bookkeeping: one engine, one node list, the content ids and the active filter column."""

    def __init__(self, nodes, engine: Optional[RetrievalEngine]):
        self.nodes = list(nodes)
        self.engine = engine if engine is not None else RetrievalEngine()
        self._classes: Optional[_MetaClasses] = None
        seen: Dict[Hashable, int] = {}
        cid = np.empty(len(self.nodes), np.int32)
        for i, n in enumerate(self.nodes):
            cid[i] = seen.setdefault(n.get_content(), i)      # smallest index with identical text
        self.content_id = cid
        self._push_meta()

    def _push_meta(self):
        self.engine.set_doc_meta(len(self.nodes), self.content_id, None if self._classes is None else self._classes.ids)

    def filter_class(self, filter_dict: Optional[Dict[str, Any]]) -> int:
        """Class id of `filter_dict` in the column over ITS key set.  The device holds one column at a time; the host tables
        are kept per key set, so alternating between two key sets (filter_dict on one route, filters on the other with
        different keys) costs the 2-bytes-per-node upload but not the walk over all nodes' metadata."""
        if not filter_dict:
            return -1
        keys = tuple(sorted(filter_dict))
        if self._classes is None or self._classes.keys != keys:
            cache = self.__dict__.setdefault("_class_tables", {})
            if keys not in cache:
                cache[keys] = _MetaClasses(self.nodes, keys)
            self._classes = cache[keys]
            self._push_meta()
        return self._classes.class_of(filter_dict)

    def _use_keys(self, keys: tuple) -> "_MetaClasses":
        if self._classes is None or self._classes.keys != keys:
            cache = self.__dict__.setdefault("_class_tables", {})
            if keys not in cache:
                cache[keys] = _MetaClasses(self.nodes, keys)
            self._classes = cache[keys]
            self._push_meta()
        return self._classes

    def too_many_values(self, keys: tuple) -> bool:
        """True when the nodes carry more distinct value tuples over `keys` than a class column can number (the walk that finds out
        runs once per key set; the table it builds otherwise is the one the class-column path uses)."""
        known = self.__dict__.setdefault("_too_many", {})
        if keys not in known:
            cache = self.__dict__.setdefault("_class_tables", {})
            try:
                if keys not in cache:
                    cache[keys] = _MetaClasses(self.nodes, keys)
                known[keys] = False
            except _TooManyClasses:
                known[keys] = True
        return known[keys]

    def rows_matching(self, spec) -> np.ndarray:
        """Ascending row ids whose metadata satisfies `spec` (a dict of the equality shape or a _SetFilter), by evaluating the filter on
        every node: an O(N) host walk per DISTINCT filter, cached like class_set's evaluations.  For key sets without a class table."""
        key = ("eq", tuple(sorted(spec.items(), key=repr))) if isinstance(spec, dict) else spec.node
        cache = self.__dict__.setdefault("_rows_cache", {})
        hit = cache.get(key)
        if hit is None:
            if isinstance(spec, dict):                     # the class column's equality: an absent key equals None
                items = list(spec.items())
                keep = [i for i, n in enumerate(self.nodes) if all(n.metadata.get(k) == v for k, v in items)]
            else:
                keys = spec.keys
                keep = [i for i, n in enumerate(self.nodes)
                        if _holds(spec.node, {k: n.metadata[k] for k in keys if n.metadata.get(k) is not None})]
            hit = np.asarray(keep, np.int64)
            if len(cache) >= 256:
                cache.clear()
            cache[key] = hit
        return hit

    def class_rows(self, table: "_MetaClasses", c: int) -> np.ndarray:
        """Ascending rows of class c of `table`, cached per class table."""
        cache = table.__dict__.setdefault("_rows_of_class", {})
        hit = cache.get(c)
        if hit is None:
            hit = cache[c] = np.flatnonzero(table.ids == c).astype(np.int64)
        return hit

    def class_counts(self, table: "_MetaClasses") -> np.ndarray:
        cnt = table.__dict__.get("_counts")
        if cnt is None:
            cnt = table.__dict__["_counts"] = np.bincount(table.ids.astype(np.int64), minlength=len(table.values))
        return cnt

    def class_set(self, spec: "_SetFilter") -> Optional[List[int]]:
        """Classes (of the column over spec.keys) whose value tuple satisfies the filter, ascending; None = every class.  The
        evaluation is cached per class table and compiled filter: the reference's loop sends the same few filters over and over."""
        if not spec.keys:
            return None if _holds(spec.node, {}) else []
        table = self._use_keys(spec.keys)
        cache = table.__dict__.setdefault("_set_cache", {})
        hit = cache.get(spec.node)
        if hit is None:
            allowed = [j for vals, j in table.values.items()
                       if _holds(spec.node, {k: v for k, v in zip(table.keys, vals) if v is not None})]
            hit = ("all",) if len(allowed) == len(table.values) else tuple(sorted(allowed))
            if len(cache) >= 4096:
                cache.clear()
            cache[spec.node] = hit
        return None if hit == ("all",) else list(hit)

    def plan(self, specs: Sequence[Any]) -> List[Any]:
        """Per query of one key-set group: -1 (unfiltered), a class id (today's column path), or a list of >= 2 class ids; [] = no
        row can match (the query returns nothing without a scan).  Dicts keep today's classes (32767 = matches nothing)."""
        out: List[Any] = []
        for sp in specs:
            if not sp:
                out.append(-1)
            elif isinstance(sp, dict):
                out.append(self.filter_class(sp))
            else:
                cs = self.class_set(sp)
                out.append(-1 if cs is None else (cs[0] if len(cs) == 1 else cs))
        return out

    def filter_column(self, filter_dicts: Sequence[Optional[Dict[str, Any]]]) -> Optional[np.ndarray]:
        """int16[B] class column for a batch whose queries carry their OWN filters (None / {} = unfiltered: -1), or None
        when no query is filtered.  All filters of one column use one metadata key set (the device holds one class
        column at a time); `_by_key_set` splits batches that mix key sets."""
        keys = {tuple(sorted(fd)) for fd in filter_dicts if fd}
        if not keys:
            return None
        if len(keys) > 1:
            raise ValueError("the filters of one device batch must share their metadata keys")
        col = np.full(len(filter_dicts), -1, np.int16)
        for b, fd in enumerate(filter_dicts):
            if fd:
                col[b] = self.filter_class(fd)
        return col


_UNSET = object()      # "argument not given": the retriever's scalar attribute (filters / filter_dict) applies to every query


def _per_query(value, B: int, to_dict) -> List[Optional[Dict[str, Any]]]:
    """One filter per query.  `value` is the reference's scalar knob (None, a {key: value} dict, a qdrant Filter: applies
    to every query, as `retriever.filters = ...` / `.filter_dict = ...` do, ref pipeline.py:333-341) or a list / tuple
    parallel to the queries (the reference's evaluation loop sets a new filter before every question, main.py:48-52 ->
    pipeline.py:301-312: a batch of its questions carries one filter EACH)."""
    if isinstance(value, (list, tuple)):
        if len(value) != B:
            raise ValueError(f"per-query filters: {len(value)} filters for {B} queries")
        return [to_dict(v) for v in value]
    one = to_dict(value)
    return [one] * B


def _by_key_set(dicts: Sequence[Optional[Dict[str, Any]]]) -> List[List[int]]:
    """Query positions grouped so that each group's filters share one metadata key set (unfiltered queries join the
    first group).  The usual batch -- every filter on `dir` -- is ONE group."""
    groups: Dict[tuple, List[int]] = {}
    free: List[int] = []
    for b, fd in enumerate(dicts):
        keys = _spec_keys(fd)          # (a set filter's key set = every key it mentions; a constant one needs no column)
        if keys:
            groups.setdefault(keys, []).append(b)
        else:
            free.append(b)
    out = list(groups.values())
    if not out:
        return [free] if free else []
    out[0] = sorted(out[0] + free)
    return out


def _per_query_rows(rows, B: int, n: int) -> List[Optional[np.ndarray]]:
    """`rows` (one id array for every query, or a list parallel to the queries of arrays / None) -> per query None or an ascending,
    duplicate-free int64 array inside [0, n); the same input object gives the same array object.  Both routes normalise with this."""
    if rows is None:
        return [None] * B
    seen: Dict[int, tuple] = {}

    def norm(a):
        hit = seen.get(id(a))
        if hit is None:
            arr = np.unique(np.asarray(a).reshape(-1).astype(np.int64))
            if arr.size and (arr[0] < 0 or arr[-1] >= n):
                raise ValueError(f"rows must lie in [0, {n})")
            hit = seen[id(a)] = (a, arr)               # (a is held, so its id stays its own for the call)
        return hit[1]
    per_query = (isinstance(rows, (list, tuple)) and len(rows) == B
                 and all(r is None or (hasattr(r, "__len__") and not isinstance(r, (str, bytes))) for r in rows))
    if per_query:
        return [None if r is None else norm(r) for r in rows]
    one = norm(rows)
    return [one] * B


def _rows_lists(rows_q: Sequence[np.ndarray]):
    """Row arrays of the queries -> (distinct lists, list_of): identical arrays, by object identity or by content, become one list."""
    lists: List[np.ndarray] = []
    by_id: Dict[int, int] = {}
    by_content: Dict[tuple, int] = {}
    list_of = np.empty(len(rows_q), np.int32)
    for j, r in enumerate(rows_q):
        l = by_id.get(id(r))
        if l is None:
            key = (r.shape[0], r.tobytes())
            l = by_content.get(key)
            if l is None:
                l = by_content[key] = len(lists)
                lists.append(r)
            by_id[id(r)] = l
        list_of[j] = l
    return lists, list_of


def _node_positions(holder, nodes, nodes_or_ids, owner: str) -> np.ndarray:
    """Positions in `nodes` of the given positions / node objects (NodeWithScore included), ascending and distinct.  The object ->
    position map is built on first use and kept on `holder`."""
    where = holder.__dict__.get("_position")
    ids = []
    for x in nodes_or_ids:
        if isinstance(x, (int, np.integer)):
            ids.append(int(x))
            continue
        if where is None:
            where = holder.__dict__["_position"] = {id(n): i for i, n in enumerate(nodes)}
        node = getattr(x, "node", x)
        if id(node) not in where:
            raise ValueError(f"score_nodes: a node that is not part of this {owner}'s node list")
        ids.append(where[id(node)])
    return np.unique(np.asarray(ids, np.int64))


# ---------------------------------------------------------------------------------------------------
# Exclude lists (DESIGN K12): `exclude=` of the retrievers and must_not: [HasIdCondition] of their filters.
def plan_exclusion(k: int, e_max: int, limit: int) -> str:
    """Which route serves top k minus an exclusion list of e_max ids on a route whose depth limit is `limit`: "drop" -- the route's
    pipeline at depth k + e_max and the drop kernel (erh_*_topk_excl) -- when that depth fits, else "complement": the allowed rows
    without the excluded ones as a rows= list (erh_*_topk_rows).  The result is the same either way."""
    return "drop" if int(k) + int(e_max) <= int(limit) else "complement"


def _id_positions(holder, nodes, entry, owner: str) -> np.ndarray:
    """Positions in `nodes` of one exclude / HasIdCondition entry -- positions, node ids (strings), node objects or NodeWithScore, in
    any mixture --, ascending and distinct.  The node id -> position map is built on first use and kept on `holder`."""
    if entry is None:
        return np.zeros(0, np.int64)
    if isinstance(entry, np.ndarray):
        entry = entry.reshape(-1).tolist() if entry.dtype.kind in "iu" else list(entry.reshape(-1))
    elif isinstance(entry, (str, bytes)) or not hasattr(entry, "__iter__"):
        entry = [entry]
    out, objs = [], []
    for x in entry:
        if isinstance(x, str):
            by_id = holder.__dict__.get("_position_of_id")
            if by_id is None:
                by_id = holder.__dict__["_position_of_id"] = {n.node_id: i for i, n in enumerate(nodes)}
            if x not in by_id:
                raise ValueError(f"exclude: node id {x!r} is not part of this {owner}'s node list")
            out.append(by_id[x])
        elif isinstance(x, (int, np.integer)) and not isinstance(x, bool):
            if not 0 <= int(x) < len(nodes):
                raise ValueError(f"exclude: positions must lie in [0, {len(nodes)})")
            out.append(int(x))
        else:
            objs.append(x)
    pos = np.asarray(out, np.int64)
    if objs:
        pos = np.concatenate([pos, _node_positions(holder, nodes, objs, owner)])
    return np.unique(pos)


def _per_query_exclude(exclude, B: int, resolve) -> Optional[List[np.ndarray]]:
    """`exclude` (one entry for every query, or a list parallel to the queries of entries / None) -> per query an ascending,
    duplicate-free position array; None when nothing is given.  `resolve(entry)` is _id_positions on the caller's nodes."""
    if exclude is None:
        return None
    per_query = (isinstance(exclude, (list, tuple)) and len(exclude) == B
                 and all(e is None or (hasattr(e, "__len__") and not isinstance(e, (str, bytes))) for e in exclude))
    if per_query:
        return [resolve(e) for e in exclude]
    one = resolve(exclude)
    return [one] * B


class _RestFilter:
    """A Filter without its top-level id conditions: what the payload compiler (_filter_spec) gets."""

    __slots__ = ("must", "should", "must_not", "min_should")

    def __init__(self, must, should, must_not, min_should):
        self.must, self.should, self.must_not, self.min_should = must, should, must_not, min_should


def _split_id_conditions(f):
    """One filter -> (the filter without the HasIdCondition entries of its top-level must / must_not, the ids every must entry lists
    (None: no such entry), the ids any must_not entry lists (None: no such entry)).  A HasIdCondition anywhere else stays where it is
    and the payload compiler raises its TypeError there."""
    if f is None or isinstance(f, dict) or not any(hasattr(f, a) for a in ("must", "should", "must_not")):
        return f, None, None
    must, must_not = _clause(getattr(f, "must", None)), _clause(getattr(f, "must_not", None))
    inc = [c for c in must if hasattr(c, "has_id")]
    exc = [c for c in must_not if hasattr(c, "has_id")]
    if not inc and not exc:
        return f, None, None
    rest = _RestFilter([c for c in must if not hasattr(c, "has_id")], getattr(f, "should", None),
                       [c for c in must_not if not hasattr(c, "has_id")], getattr(f, "min_should", None))
    return rest, ([list(_clause(c.has_id)) for c in inc] or None), ([x for c in exc for x in _clause(c.has_id)] if exc else None)


def _has_id_conditions(filters) -> bool:
    """Whether a filter (or one of a list of filters) carries a HasIdCondition in its top-level must / must_not."""
    return any(_split_id_conditions(f)[1:] != (None, None) for f in (filters if isinstance(filters, (list, tuple)) else [filters]))


def _lift_id_conditions(filters, rows, exclude, B: int, n: int, resolve):
    """The HasIdCondition entries of a batch's filters moved to where they are served: must -> the query's rows= list (the ids every
    entry lists; with a rows= argument as well: those of them), must_not -> its exclusion (with an exclude= argument as well: both).
    Returns (filters, rows, exclude per query or None); a batch without id conditions gets its `filters` and `rows` back untouched."""
    excl_q = _per_query_exclude(exclude, B, resolve)
    per = list(filters) if isinstance(filters, (list, tuple)) and len(filters) == B else None
    seen: Dict[int, tuple] = {}

    def split(f):
        hit = seen.get(id(f))
        if hit is None:
            hit = seen[id(f)] = (f, _split_id_conditions(f))     # (f is held, so its id stays its own for the batch)
        return hit[1]
    parts = [split(f) for f in (per if per is not None else [filters])]
    if all(m is None and x is None for _, m, x in parts):
        return filters, rows, excl_q
    if per is None:
        parts = parts * B
    rows_q = _per_query_rows(rows, B, n)
    if excl_q is None:
        excl_q = [np.zeros(0, np.int64)] * B
    excl_q = list(excl_q)
    for b, (_, m, x) in enumerate(parts):
        if m is not None:
            for ids in m:
                r = resolve(ids)
                rows_q[b] = r if rows_q[b] is None else np.intersect1d(rows_q[b], r, assume_unique=True)
        if x is not None:
            excl_q[b] = np.union1d(excl_q[b], resolve(x))
    return [rest for rest, _, _ in parts], (rows_q if any(r is not None for r in rows_q) else None), excl_q


def _without(rows: np.ndarray, excl: np.ndarray) -> np.ndarray:
    return rows if excl.size == 0 else rows[~np.isin(rows, excl)]


def _allowed_rows(corpus: "_FilteredCorpus", spec) -> np.ndarray:
    """Ascending rows a query with filter `spec` (None, a dict, a _SetFilter) may see: the complement route's population."""
    return np.arange(len(corpus.nodes), dtype=np.int64) if not spec else corpus.rows_matching(spec)


def _plan_sets(plan: Sequence[Any]):
    """corpus.plan's answers as the class sets of an erh_*_topk_excl call; None when no query is filtered."""
    if all(not isinstance(c, list) and c == -1 for c in plan):
        return None
    return [None if (not isinstance(c, list) and c == -1) else (c if isinstance(c, list) else [c]) for c in plan]


def _corpus_for(nodes, engine: Optional[RetrievalEngine]) -> _FilteredCorpus:
    """Retrievers built over the same engine share one _FilteredCorpus (and so one metadata upload).  The
    bookkeeping lives on the engine object (no process-global cache pinning engines); an engine serves ONE node
    list -- the same node objects in the same order -- and anything else is an error, not a silent reuse."""
    if engine is not None and engine.corpus is not None:
        c = engine.corpus
        nodes = list(nodes)
        if len(c.nodes) != len(nodes) or any(a is not b for a, b in zip(c.nodes, nodes)):
            raise ValueError("this RetrievalEngine already serves a different node list; use one engine per corpus")
        return c
    c = _FilteredCorpus(nodes, engine)
    c.engine.corpus = c
    return c


# ---------------------------------------------------------------------------------------------------
class HipVectorStore:
    """Stand-in for the Qdrant collection (Distance.COSINE, ref ingestion.py:155-191): the chunk embeddings
    live as one fp16 matrix in HBM.  `embeddings` is [N, d] (numpy or torch, fp16/fp32), row i belongs to
    nodes[i]; normalize=True applies Qdrant's insert-time L2 normalisation."""

    def __init__(self, nodes, embeddings, engine: Optional[RetrievalEngine] = None, normalize: bool = True):
        self.corpus = _corpus_for(nodes, engine)
        self.engine = self.corpus.engine
        is_f16 = str(getattr(embeddings, "dtype", "")).endswith("float16")
        if normalize and not is_f16 and isinstance(embeddings, np.ndarray):
            self.engine.set_dense(_unit_f16(embeddings))             # host: fp16 rounding of the unit rows is pinned
        else:
            self.engine.set_dense(embeddings, normalize=normalize and not is_f16)   # device tensors: normalise on the GPU

    @property
    def nodes(self):
        return self.corpus.nodes

    # -- restart path ---------------------------------------------------------------------------------------------------
    # The reference embeds the corpus ONCE: when the Qdrant collection is already populated it skips ingestion
    # (ref pipeline.py:138-141, `collection_info.points_count == 0`), so after a restart the embeddings exist only in
    # Qdrant.  Two ways to come back without re-embedding: read them out of that collection (from_qdrant / afrom_qdrant),
    # or keep the fp16 matrix this store scores with in a file of its own (save / load).  These are loaders, not a storage
    # engine: one pass, then everything is resident in HBM as before.
    @staticmethod
    def _point_fields(point):
        """(id, vector, text, metadata) of one scrolled Qdrant point as llama-index-vector-stores-qdrant==0.2.0 writes it
        (ref requirements.txt:49; UNPINNED offline: point id = node_id, payload = flat metadata + `_node_content`, the
        node's JSON).  Named-vector collections hand back {name: vector}: the single entry is taken."""
        import json
        payload = getattr(point, "payload", None) or {}
        vec = getattr(point, "vector", None)
        if isinstance(vec, dict):
            if len(vec) != 1:
                raise ValueError("point carries several named vectors; pass vectors through a client wrapper that selects one")
            vec = next(iter(vec.values()))
        text, meta = payload.get("text"), None
        content = payload.get("_node_content")
        if content:
            node_json = json.loads(content) if isinstance(content, str) else dict(content)
            text = node_json.get("text", text)
            meta = node_json.get("metadata")
        if meta is None:
            meta = {k: v for k, v in payload.items() if not k.startswith("_") and k not in ("text", "document_id", "doc_id", "ref_doc_id")}
        return getattr(point, "id", None), vec, text, meta

    class _Scroll:
        """What a scroll over the collection leaves behind: per point its id, text and metadata, and the vectors as one float32
        block per scrolled batch -- a point's vector never stays around as a Python list (3584 floats are ~115 KB of objects:
        ~10 GB for 100k chunks), and a point without its vector is reported by the batch that carries it."""

        def __init__(self):
            self.meta: List[tuple] = []
            self.blocks: List[np.ndarray] = []
            self.d: Optional[int] = None

        def add(self, batch) -> None:
            rows = []
            for p in batch:
                pid, vec, text, meta = HipVectorStore._point_fields(p)
                if vec is None:
                    raise ValueError(f"point {pid!r} came back without its vector (scroll with with_vectors=True)")
                if self.d is None:
                    self.d = len(vec)
                if len(vec) != self.d:
                    raise ValueError("points of different vector sizes in one collection")
                rows.append(vec)
                self.meta.append((pid, text, meta))
            if rows:
                self.blocks.append(np.asarray(rows, dtype=np.float32))

        def row(self, j: int, starts) -> np.ndarray:
            b = int(np.searchsorted(starts, j, side="right")) - 1
            return self.blocks[b][j - starts[b]]

    @classmethod
    def _assemble(cls, scroll: "HipVectorStore._Scroll", nodes, engine, normalize):
        """Scrolled points -> (nodes, [N, d] float32 rows aligned with them).  With `nodes` given every node must find its
        vector: by point id == node_id when all ids match, otherwise by text content -- the key the reference itself joins
        the two routes on (RRF / fusion key = get_content(), ref retrievers.py:245,263): its sparse-route nodes come from a
        second run of the splitter (pipeline.py:160-167) and share no ids with the ingested points.  Among nodes with equal
        text a point with equal `file_path` is preferred, then first come first served.  Without `nodes` the node list is
        rebuilt from the payloads in scroll order (what the reference's QdrantRetriever returns)."""
        fields = scroll.meta
        if not fields:
            raise ValueError("the collection is empty (points_count == 0): run the ingestion first, as the reference does")
        d = int(scroll.d)
        if nodes is None:
            nodes = [TextNode(text=t or "", metadata=dict(m or {}), id_=str(pid)) for pid, t, m in fields]
            return cls(nodes, np.concatenate(scroll.blocks) if len(scroll.blocks) > 1 else scroll.blocks[0], engine=engine, normalize=normalize)
        nodes = list(nodes)
        by_id = {str(pid): j for j, (pid, _, _) in enumerate(fields)}
        if len(by_id) == len(fields) and all(str(n.node_id) in by_id for n in nodes):
            order = [by_id[str(n.node_id)] for n in nodes]
        else:
            by_text: Dict[Any, List[int]] = {}
            for j, (_, t, _) in enumerate(fields):
                by_text.setdefault(t, []).append(j)
            order, missing = [], 0
            for n in nodes:
                bucket = by_text.get(n.get_content())
                if not bucket:
                    missing += 1
                    order.append(-1)
                    continue
                fp = n.metadata.get("file_path")
                pick = next((j for j in bucket if (fields[j][2] or {}).get("file_path") == fp), bucket[0])
                bucket.remove(pick)
                order.append(pick)
            if missing:
                raise ValueError(f"{missing} of {len(nodes)} nodes have no point with their text in the collection "
                                 f"({len(fields)} points): the collection was built from a different corpus / splitter")
        starts = np.cumsum([0] + [blk.shape[0] for blk in scroll.blocks])[:-1]
        emb = np.empty((len(nodes), d), np.float32)                   # the one full-size array; filled block row by block row
        for i, j in enumerate(order):
            emb[i] = scroll.row(j, starts)
        return cls(nodes, emb, engine=engine, normalize=normalize)

    @classmethod
    def from_qdrant(cls, client, collection_name: str, nodes=None, engine: Optional[RetrievalEngine] = None,
                    batch_size: int = 1024, normalize: bool = True) -> "HipVectorStore":
        """The chunk matrix out of an already populated Qdrant collection (a synchronous `QdrantClient`, or anything with its
        `scroll(collection_name=, limit=, offset=, with_payload=, with_vectors=) -> (points, next_offset)`)."""
        scroll, offset = cls._Scroll(), None
        while True:
            res = client.scroll(collection_name=collection_name, limit=batch_size, offset=offset, with_payload=True,
                                with_vectors=True)
            if hasattr(res, "__await__"):
                if hasattr(res, "close"):
                    res.close()
                raise TypeError("this client's scroll() is a coroutine (AsyncQdrantClient): use `await HipVectorStore.afrom_qdrant(...)`")
            batch, offset = res
            scroll.add(batch)
            if offset is None or not batch:
                break
        return cls._assemble(scroll, nodes, engine, normalize)

    @classmethod
    async def afrom_qdrant(cls, client, collection_name: str, nodes=None, engine: Optional[RetrievalEngine] = None,
                           batch_size: int = 1024, normalize: bool = True) -> "HipVectorStore":
        """from_qdrant for the `AsyncQdrantClient` the reference's pipeline holds (ref ingestion.py:163-169)."""
        scroll, offset = cls._Scroll(), None
        while True:
            batch, offset = await client.scroll(collection_name=collection_name, limit=batch_size, offset=offset,
                                                with_payload=True, with_vectors=True)
            scroll.add(batch)
            if offset is None or not batch:
                break
        return cls._assemble(scroll, nodes, engine, normalize)

    @staticmethod
    def _fingerprint(nodes) -> str:
        import hashlib
        h = hashlib.sha256()
        for n in nodes:
            t = n.get_content().encode("utf-8", "surrogatepass")
            h.update(len(t).to_bytes(8, "little"))
            h.update(t)
        return h.hexdigest()

    @staticmethod
    def _paths(path):
        path = str(path)
        if not path.endswith(".npy"):
            path += ".npy"
        return path, path + ".meta.json"

    def save(self, path) -> str:
        """Write the resident matrix -- the unit-norm fp16 rows the kernels score, in node order -- as `<path>.npy` plus a
        small `<path>.npy.meta.json` (shape and a fingerprint of the node texts, checked by load).  2 bytes per element."""
        import json
        npy, meta = self._paths(path)
        eng = self.engine
        n, d = int(eng.n_dense), int(eng.d)
        if n != len(self.corpus.nodes):
            raise ValueError("the engine's chunk matrix does not belong to this store's nodes")
        mm = np.lib.format.open_memmap(npy, mode="w+", dtype=np.float16, shape=(n, d))
        slab = max(1, (64 << 20) // (2 * d))
        for r0 in range(0, n, slab):
            rows = min(slab, n - r0)
            eng.get_dense_rows(r0, rows, out=mm[r0:r0 + rows])
        mm.flush()
        del mm
        with open(meta, "w") as f:
            json.dump({"format": "easyrag_amd.HipVectorStore/1", "n": n, "d": d, "dtype": "float16", "unit_norm": True,
                       "nodes_sha256": self._fingerprint(self.corpus.nodes)}, f)
        return npy

    @classmethod
    def load(cls, path, nodes, engine: Optional[RetrievalEngine] = None, check: bool = True) -> "HipVectorStore":
        """The store of a previous process over the same nodes: rows go to the device as they were saved (no re-normalisation,
        no re-rounding), so every result is bit-identical to the process that saved them."""
        import json
        npy, meta = cls._paths(path)
        with open(meta) as f:
            info = json.load(f)
        nodes = list(nodes)
        if info.get("format") != "easyrag_amd.HipVectorStore/1" or info.get("dtype") != "float16":
            raise ValueError(f"{meta}: not a HipVectorStore file")
        if int(info["n"]) != len(nodes):
            raise ValueError(f"{npy} holds {info['n']} rows, the node list has {len(nodes)}")
        if check and info.get("nodes_sha256") != cls._fingerprint(nodes):
            raise ValueError(f"{npy} was saved for different node texts (fingerprint mismatch); pass check=False to override")
        x = np.load(npy, mmap_mode="r")
        if x.dtype != np.float16 or x.shape != (int(info["n"]), int(info["d"])):
            raise ValueError(f"{npy}: shape / dtype differ from its meta file")
        return cls(nodes, x, engine=engine, normalize=False)

    rows_route_max = 0     # > 0: a filtered query whose filter allows at most this many rows goes through the rows entry (opt-in; results identical)

    def query_batch(self, query_embeddings, similarity_top_k: int, filters=None, mode: int = _lib.ERH_DENSE_EXACT, rows=None,
                    exclude=None):
        """`filters`: one filter for the whole batch (None, dict, qdrant Filter) or a list with one filter per query.
        `rows`: restrict queries to explicit row ids (positions in the node list) -- one id array for every query, or a list parallel to
        the queries whose entries are an id array or None.  Such a query ranks exactly those rows (erh_dense_topk_rows; with a filter as
        well: the rows that also pass it), the others run as without the argument, and the two parts are scattered into one result.
        `exclude`: node positions a query must NOT return -- one array for every query, or a list parallel to the queries of arrays /
        None: the top k of (what the filter and rows allow) minus those (erh_dense_topk_excl, or the complement as a rows list where
        k + the list's length exceeds the call's depth: plan_exclusion)."""
        q = _unit_f16(query_embeddings)
        B, k = q.shape[0], int(similarity_top_k)
        if not 1 <= k <= DENSE_MAX_K:
            # no exact host fall-back: the chunk matrix lives on the device only
            raise ValueError(f"dense similarity_top_k must lie in [1, {DENSE_MAX_K}], got {k}")
        if rows is not None and mode != _lib.ERH_DENSE_EXACT:
            raise ValueError("rows= ranks by the pinned fp64 score of every listed row: ERH_DENSE_EXACT only")
        dicts = _per_query(filters, B, _spec_cache())
        rows_q, dicts = self._resolve_rows(dicts, rows, B, mode)
        excl_q = _per_query_exclude(exclude, B, lambda e: _id_positions(self, self.corpus.nodes, e, "store"))
        if excl_q is not None and any(e.size for e in excl_q):
            return self._query_excluding(q, k, dicts, rows_q, excl_q, mode)
        with_rows = [b for b in range(B) if rows_q[b] is not None]
        if not with_rows:
            return self._query_filtered(q, k, dicts, mode)
        lists, list_of = self._rows_lists([rows_q[b] for b in with_rows])
        if len(with_rows) == B:
            return self.engine.dense_topk_rows(q, k, lists, list_of=list_of)
        ids, sc, ln = np.full((B, k), -1, np.int32), np.zeros((B, k), np.float64), np.zeros(B, np.int32)
        rest = [b for b in range(B) if rows_q[b] is None]
        ids[rest], sc[rest], ln[rest] = self._query_filtered(q[rest], k, [dicts[b] for b in rest], mode)
        ids[with_rows], sc[with_rows], ln[with_rows] = self.engine.dense_topk_rows(q[with_rows], k, lists, list_of=list_of)
        return ids, sc, ln

    def _query_excluding(self, q, k: int, dicts, rows_q, excl_q, mode: int):
        """The batch with exclusion lists.  A query with rows ranks its rows without the excluded ones; any other takes the drop route
        (erh_dense_topk_excl, the filter as the call's class sets) when k + its exclusions fit the call's depth, else the complement
        route: the rows its filter allows without the excluded ones, as a rows list."""
        B = q.shape[0]
        rows_q = list(rows_q)
        drop: List[int] = []
        for b in range(B):
            if rows_q[b] is not None:
                rows_q[b] = _without(rows_q[b], excl_q[b])
            elif plan_exclusion(k, excl_q[b].size, DENSE_MAX_K) == "drop":
                drop.append(b)
            else:
                if mode != _lib.ERH_DENSE_EXACT:
                    raise ValueError(f"an exclusion list of {excl_q[b].size} ids with k = {k} exceeds the depth of erh_dense_topk_excl "
                                     f"({DENSE_MAX_K}) and takes the rows route: ERH_DENSE_EXACT only")
                rows_q[b] = _without(_allowed_rows(self.corpus, dicts[b]), excl_q[b])
        ids, sc, ln = np.full((B, k), -1, np.int32), np.zeros((B, k), np.float64), np.zeros(B, np.int32)
        for g in _by_key_set([dicts[b] for b in drop]):
            g = [drop[j] for j in g]
            sets = _plan_sets(self.corpus.plan([dicts[b] for b in g]))
            ids[g], sc[g], ln[g] = self.engine.dense_topk_excl(q[g], k, [excl_q[b] for b in g], sets=sets, mode=mode)
        with_rows = [b for b in range(B) if rows_q[b] is not None]
        if with_rows:
            lists, list_of = self._rows_lists([rows_q[b] for b in with_rows])
            ids[with_rows], sc[with_rows], ln[with_rows] = self.engine.dense_topk_rows(q[with_rows], k, lists, list_of=list_of)
        return ids, sc, ln

    def _per_query_rows(self, rows, B: int) -> List[Optional[np.ndarray]]:
        return _per_query_rows(rows, B, len(self.corpus.nodes))

    def _resolve_rows(self, dicts, rows, B: int, mode: int):
        """Per query the rows it may rank (None: it runs through today's filter paths) and the filters left for those paths.  A query
        with rows AND a filter keeps the rows that pass the filter (class column lookup on the host); a filter over more distinct values
        than a class column holds becomes the rows it matches; with rows_route_max > 0 so does a filter that allows few rows."""
        rows_q = self._per_query_rows(rows, B)
        dicts = list(dicts)
        corpus = self.corpus
        exact = mode == _lib.ERH_DENSE_EXACT
        if rows is None and not (exact and (self.rows_route_max > 0 or any(dicts))):
            return rows_q, dicts
        for g in _by_key_set(dicts):
            for b in g:
                sp = dicts[b]
                if not sp:
                    continue
                keys = _spec_keys(sp)
                if keys and exact and corpus.too_many_values(keys):
                    allowed = corpus.rows_matching(sp)
                    rows_q[b] = allowed if rows_q[b] is None else np.intersect1d(rows_q[b], allowed, assume_unique=True)
                    dicts[b] = None
                    continue
                if rows_q[b] is None and not (exact and self.rows_route_max > 0):
                    continue
                # the filter as classes of the column over its keys: -1 everything, a class, a list of classes ([] nothing)
                c = corpus.plan([sp])[0]
                table = corpus._classes
                if rows_q[b] is not None:
                    r = rows_q[b]
                    if isinstance(c, list) and not c:
                        r = r[:0]
                    elif c != -1:
                        r = r[np.isin(table.ids[r], np.asarray(c if isinstance(c, list) else [c], np.int64))]
                    rows_q[b], dicts[b] = r, None
                elif c != -1 and not (isinstance(c, list) and not c) and c != 32767:
                    cs = c if isinstance(c, list) else [c]
                    if int(corpus.class_counts(table)[cs].sum()) <= self.rows_route_max:
                        parts = [corpus.class_rows(table, int(x)) for x in cs]
                        rows_q[b] = parts[0] if len(parts) == 1 else np.sort(np.concatenate(parts))
                        dicts[b] = None
        return rows_q, dicts

    _rows_lists = staticmethod(_rows_lists)        # (the module-level helper both routes share)

    def _query_filtered(self, q, k: int, dicts, mode: int):
        """The batch through the filter paths: class column, class sets, one device column per metadata key set."""
        B = q.shape[0]
        groups = _by_key_set(dicts)
        has_sets = any(isinstance(sp, _SetFilter) for sp in dicts)
        if len(groups) <= 1 and not has_sets:
            return self.engine.dense_topk(q, k, filter_dir=self.corpus.filter_column(dicts), mode=mode)
        ids, sc, ln = np.full((B, k), -1, np.int32), np.zeros((B, k), np.float64), np.zeros(B, np.int32)
        for g in groups:                              # filters over different metadata keys: one device column at a time
            if has_sets:
                gi, gs, gl = self._query_planned(q[g], k, self.corpus.plan([dicts[b] for b in g]), mode)
            else:
                gi, gs, gl = self.engine.dense_topk(q[g], k, filter_dir=self.corpus.filter_column([dicts[b] for b in g]), mode=mode)
            ids[g], sc[g], ln[g] = gi, gs, gl
        return ids, sc, ln

    def _query_planned(self, q, k: int, plan: List[Any], mode: int):
        """One key-set group after corpus.plan: queries whose filter matches no row get nothing (no scan); a group without a
        set of two or more classes is today's class-column call, any other erh_dense_topk_sets."""
        B = len(plan)
        live = [b for b in range(B) if not (isinstance(plan[b], list) and not plan[b])]
        if any(isinstance(c, list) and len(c) > 1 for c in plan):
            return self.engine.dense_topk_sets(q, k, [None if c == -1 else (c if isinstance(c, list) else [c]) for c in plan],
                                               mode=mode)
        ids, sc, ln = np.full((B, k), -1, np.int32), np.zeros((B, k), np.float64), np.zeros(B, np.int32)
        if live:
            col = np.asarray([plan[b] for b in live], np.int16)
            ids[live], sc[live], ln[live] = self.engine.dense_topk(q[live], k, filter_dir=col if np.any(col >= 0) else None,
                                                                   mode=mode)
        return ids, sc, ln

    def query(self, query_embedding, similarity_top_k: int, filters=None, rows=None):
        ids, sc, ln = self.query_batch(query_embedding, similarity_top_k, filters, rows=rows)
        n = int(ln[0])
        return [self.corpus.nodes[i] for i in ids[0, :n]], [float(s) for s in sc[0, :n]]


try:  # the reference's base class (ref retrievers.py:7,23,80,223) whenever llama_index is installed
    from llama_index.core.base.base_retriever import BaseRetriever as _LlamaBaseRetriever  # type: ignore
except Exception:  # pragma: no cover - the build container has no llama_index
    _LlamaBaseRetriever = None

if _LlamaBaseRetriever is not None:
    class _RetrieverBase(_LlamaBaseRetriever):
        """llama_index's BaseRetriever itself: `retrieve` / `aretrieve` (callback events, recursive retrieval over
        `objects`) come from it, so `AutoMergingRetriever(sparse_retriever, ...)` (ref pipeline.py:212-217) and RETRIEVE
        callbacks work as with the reference's classes; this file supplies `_retrieve` / `_aretrieve`."""

        def _init_base(self, callback_manager=None, object_map=None, objects=None, verbose: bool = False) -> None:
            _LlamaBaseRetriever.__init__(self, callback_manager=callback_manager, object_map=object_map,
                                         objects=objects, verbose=verbose)
else:
    class _RetrieverBase:
        """Fallback without llama_index: the slice of BaseRetriever the pipeline uses -- retrieve / aretrieve accept str
        or QueryBundle; the ctor arguments of the real base class are kept as attributes."""

        def _init_base(self, callback_manager=None, object_map=None, objects=None, verbose: bool = False) -> None:
            self.callback_manager = callback_manager
            self.object_map = object_map or {}
            self.objects = objects
            self._verbose = verbose

        def retrieve(self, str_or_query_bundle) -> List[NodeWithScore]:
            return self._retrieve(_as_bundle(str_or_query_bundle))

        async def aretrieve(self, str_or_query_bundle) -> List[NodeWithScore]:
            return await self._aretrieve(_as_bundle(str_or_query_bundle))

        async def _aretrieve(self, query_bundle: QueryBundle) -> List[NodeWithScore]:
            return self._retrieve(query_bundle)


class QdrantRetriever(_RetrieverBase):
    def __init__(self, vector_store: HipVectorStore, embed_model, similarity_top_k: int = 2, filters=None) -> None:
        self._vector_store = vector_store
        self._embed_model = embed_model
        self._similarity_top_k = similarity_top_k
        self.filters = filters
        self._init_base()

    def _retrieve(self, query_bundle: QueryBundle) -> List[NodeWithScore]:
        emb = self._embed_model.get_query_embedding(query_bundle.query_str)
        nodes, sims = self._vector_store.query(emb, self._similarity_top_k, self.filters)
        return [NodeWithScore(node=n, score=s) for n, s in zip(nodes, sims)]

    def retrieve_batch(self, queries: Sequence[str], filters=_UNSET, rows=None, exclude=None) -> List[List[NodeWithScore]]:
        """`_retrieve` for a batch.  `filters` (default: the `filters` attribute, for every query) may be a list parallel to
        `queries`: one qdrant Filter / dict / None per question, as the reference's evaluation loop sets them one at a time.
        `rows`: HipVectorStore.query_batch's argument -- node positions a query is restricted to (one array, or one array / None each).
        `exclude`: what a query must NOT return -- one entry for every query, or a list parallel to the queries of entries / None; an
        entry holds node positions, node ids, nodes or NodeWithScore.  A filter's must_not: [HasIdCondition(has_id=[...])] is the same
        thing (ids: positions or node ids), its must: [HasIdCondition] a rows list; both combine with the arguments."""
        if len(queries) == 0:
            return []
        store = self._vector_store
        fl, rows, excl_q = _lift_id_conditions(self.filters if filters is _UNSET else filters, rows, exclude, len(queries),
                                               len(store.nodes), lambda e: _id_positions(store, store.nodes, e, "store"))
        embs = np.asarray([self._embed_model.get_query_embedding(q) for q in queries], dtype=np.float32)
        kw = {} if excl_q is None else {"exclude": excl_q}    # (a store without the argument keeps working for batches without exclusions)
        ids, sc, ln = store.query_batch(embs, self._similarity_top_k, fl, rows=rows, **kw)
        nodes = self._vector_store.nodes
        return [[NodeWithScore(node=nodes[i], score=float(s)) for i, s in zip(ids[b, :ln[b]], sc[b, :ln[b]])]
                for b in range(len(queries))]

    def score_nodes(self, query: str, nodes_or_ids, top_k: Optional[int] = None) -> List[NodeWithScore]:
        """The given nodes -- positions in the node list, or node objects of it (NodeWithScore included) -- and nothing else, ranked by
        the embedding: the dense twin of BM25Retriever.get_scores(query, docs).  Every node gets its exact score on the device (one
        call, the nodes in lists of at most 768, the call's limit on k); (score desc, position asc); `top_k` cuts the result."""
        store = self._vector_store
        ids = _node_positions(store, store.nodes, nodes_or_ids, "store")
        if ids.size == 0:
            return []
        chunks = [ids[i:i + DENSE_MAX_K] for i in range(0, ids.size, DENSE_MAX_K)]
        emb = np.asarray(self._embed_model.get_query_embedding(query), dtype=np.float32)
        got, sc, ln = store.query_batch(np.tile(emb, (len(chunks), 1)), len(chunks[0]), None, rows=chunks)
        got = np.concatenate([got[j, :ln[j]] for j in range(len(chunks))])
        sc = np.concatenate([sc[j, :ln[j]] for j in range(len(chunks))])
        order = np.lexsort((got, -sc))                     # (one chunk: already in this order)
        if top_k is not None:
            order = order[:max(int(top_k), 0)]
        nodes = store.nodes
        return [NodeWithScore(node=nodes[int(got[i])], score=float(sc[i])) for i in order]


class BM25Retriever(_RetrieverBase):
    def __init__(self, nodes, tokenizer: Optional[Callable], similarity_top_k: int = DEFAULT_SIMILARITY_TOP_K,
                 callback_manager=None, objects=None, object_map=None, verbose: bool = False,
                 stopwords=("",), embed_type: int = 0, bm25_type: int = 0,
                 engine: Optional[RetrievalEngine] = None, payload_on_device: bool = False,
                 device_build: bool = True) -> None:
        self._nodes = list(nodes)
        self._tokenizer = tokenizer
        self._similarity_top_k = similarity_top_k
        self.embed_type = embed_type
        self.stopwords = stopwords
        # a NativeCutter tokenises, drops stop words and numbers the tokens inside the library (erh_text_encode): no Python
        # object per token.  Any other tokenizer (jieba.Tokenizer(), as the pipeline passes) goes through its own cut().
        # (a stop word the native side cannot express -- one with a NUL inside -- sends the build through the Python loop)
        native_text = device_build and hasattr(tokenizer, "encode_texts") and not self._str_stopwords(stopwords)[1]
        self._corpus = None if native_text else [
            tokenize_and_remove_stopwords(tokenizer, get_node_content(n, embed_type), stopwords) for n in self._nodes]
        self.bm25_type = bm25_type
        self.k1, self.b, self.epsilon = 1.5, 0.75, 0.25          # ref retrievers.py:103-105
        self._corpus_state = _corpus_for(self._nodes, engine)
        self.engine = self._corpus_state.engine
        # every retriever owns one BM25 index slot of the (possibly shared) engine: the content retriever and the
        # know_path retriever of the reference pipeline (pipeline.py:187-210) live side by side
        self._slot = self.engine.alloc_bm25_slot()
        variant = 1 if bm25_type == 1 else 0
        if device_build:
            # tokens -> ids on the host (dictionary lookups), everything else of the index build on the GPU
            # (erh_build_bm25_index: sort, run lengths, df, idf, payload); nothing but the vocabulary stays here
            if native_text:
                from .text import NativeVocab
                vocab = NativeVocab()
                flat, lens = tokenizer.encode_texts([get_node_content(n, embed_type) for n in self._nodes], vocab,
                                                    self._str_stopwords(stopwords)[0])
            else:
                vocab, flat, lens = vocab_ids(self._corpus)
            self.bm25: BM25Index = self.engine.build_bm25(flat, lens, max(len(vocab), 1), variant=variant, k1=self.k1,
                                                          b=self.b, epsilon=self.epsilon, slot=self._slot, fetch=False)
            self.bm25.vocab = vocab
        else:
            self.bm25 = build_bm25_index(self._corpus, variant=variant, k1=self.k1, b=self.b, epsilon=self.epsilon,
                                         compute_payload=not payload_on_device)
            self.engine.set_bm25(self.bm25, payload_on_device=payload_on_device, slot=self._slot)
        self.filter_dict = None
        self.filters = None                    # a Qdrant-style Filter for every query (retrieve_batch's `filters`); not the reference's knob
        self._init_base(callback_manager=callback_manager, object_map=object_map, objects=objects, verbose=verbose)

    @staticmethod
    def _str_stopwords(stopwords):
        """(usable stop words, the ones the native path cannot express): membership of '' never matters (no cutter emits an
        empty token); anything that is not a str can never equal a token."""
        sw = [w for w in stopwords if isinstance(w, str) and w != ""]
        return sw, [w for w in sw if "\x00" in w]

    def close(self):
        """Give the BM25 slot back to the engine."""
        if getattr(self, "_slot", None) is not None:
            self.engine.free_bm25_slot(self._slot)
            self._slot = None

    @classmethod
    def from_defaults(cls, index=None, nodes=None, docstore=None, tokenizer=None,
                      similarity_top_k: int = DEFAULT_SIMILARITY_TOP_K, verbose: bool = False,
                      stopwords=("",), embed_type: int = 0, bm25_type: int = 0, **kwargs) -> "BM25Retriever":
        if sum(bool(v) for v in (index, nodes, docstore)) != 1:
            raise ValueError("Please pass exactly one of index, nodes, or docstore.")
        if index is not None:
            docstore = index.docstore
        if docstore is not None:
            nodes = list(docstore.docs.values())
        assert nodes is not None, "Please pass exactly one of index, nodes, or docstore."
        return cls(nodes=nodes, tokenizer=tokenizer, similarity_top_k=similarity_top_k, verbose=verbose,
                   stopwords=stopwords, embed_type=embed_type, bm25_type=bm25_type, **kwargs)

    # -- scoring ----------------------------------------------------------------------------------
    def _query_ids(self, query: str, index: Optional[BM25Index] = None) -> np.ndarray:
        toks = tokenize_and_remove_stopwords(self._tokenizer, query, self.stopwords)
        if self.bm25_type == 1 and len(toks) == 0:
            raise IndexError("list index out of range")     # bm25s sniffs tokens[0] (ref behaviour)
        return (index or self.bm25).tokens_to_ids(toks)

    def get_scores(self, query: str, docs: Optional[Sequence[str]] = None) -> np.ndarray:
        """Score vector over all nodes (float64; float32 values widened for bm25_type 1).  With `docs` a
        throw-away index over those strings is built first (ref retrievers.py:131-147)."""
        if docs is None:
            return self._cast(self.engine.bm25_scores(self._query_ids(query), slot=self._slot))
        corpus = [tokenize_and_remove_stopwords(self._tokenizer, d, self.stopwords) for d in docs]
        idx = build_bm25_index(corpus, variant=1 if self.bm25_type == 1 else 0, k1=self.k1, b=self.b, epsilon=self.epsilon)
        # the throw-away index of a handful of sentences goes into the engine's scratch slot (kept across calls: no handle
        # creation, no kernel-attribute setup, no device allocation / free / synchronisation per call -- this sits on the
        # per-query path of the compressor)
        with _SCRATCH_LOCK:
            scratch = self.engine.scratch_bm25_slot()
            self.engine.set_bm25(idx, slot=scratch)
            return self._cast(self.engine.bm25_scores(self._query_ids(query, idx), slot=scratch))

    def _cast(self, s: np.ndarray) -> np.ndarray:
        return s.astype(np.float32) if self.bm25_type == 1 else s

    def filter(self, scores: np.ndarray) -> List[NodeWithScore]:
        """Host helper over a caller-supplied score vector (ref retrievers.py:191-210): descending walk
        (ties by node index), stop at score <= 0, metadata equality filter, first k.  The length check follows every
        walked node, rejected ones included, as in the reference: with similarity_top_k == 0 a rejected first node ends
        the walk with nothing, a kept one leaves the check unmet for the rest of the walk.  A node without a filtered
        metadata key does not match (the reference raises KeyError there)."""
        return self._filter_one(scores, self.filter_dict, self._similarity_top_k)

    def _filter_one(self, scores: np.ndarray, filter_dict, top_k: int, rows: Optional[np.ndarray] = None) -> List[NodeWithScore]:
        """`rows`: node positions the walk may keep (None: all); a node outside them is rejected like one the filter rejects."""
        scores = np.asarray(scores)
        order = np.lexsort((np.arange(scores.shape[0]), -scores.astype(np.float64)))
        keep = None
        if rows is not None:
            keep = np.zeros(scores.shape[0], bool)
            keep[rows] = True
        out: List[NodeWithScore] = []
        for ix in order:
            if scores[ix] <= 0:
                break
            meta = self._nodes[ix].metadata
            if (keep is None or keep[ix]) and (
                    filter_dict is None or not any(k not in meta or meta[k] != v for k, v in filter_dict.items())):
                out.append(NodeWithScore(node=self._nodes[ix], score=float(scores[ix])))
            if len(out) == top_k:
                break
        return out

    def _retrieve(self, query_bundle: QueryBundle) -> List[NodeWithScore]:
        if query_bundle.custom_embedding_strs or query_bundle.embedding:
            logger.warning("BM25Retriever does not support embeddings, skipping...")
        return self.retrieve_batch([query_bundle.query_str])[0]

    def _resolve_rows(self, dicts, rows, B: int):
        """Per query the rows it may rank (None: it runs through the class-column / class-set calls) and the filters left for those calls
        (a dict or a _SetFilter each).  A query with rows AND a filter keeps the rows that pass the filter: a host lookup in the class
        column over the filter's keys.  A filter over more distinct value tuples than a class column holds becomes the rows it matches
        (_FilteredCorpus.rows_matching), as on the dense route."""
        rows_q = _per_query_rows(rows, B, len(self._nodes))
        dicts = list(dicts)
        corpus = self._corpus_state
        for b in range(B):
            sp = dicts[b]
            if not sp:
                continue
            keys = _spec_keys(sp)
            if keys and corpus.too_many_values(keys):
                allowed = corpus.rows_matching(sp)
                rows_q[b] = allowed if rows_q[b] is None else np.intersect1d(rows_q[b], allowed, assume_unique=True)
                dicts[b] = None
            elif rows_q[b] is not None:
                c = corpus.plan([sp])[0]       # -1 everything, a class (32767: no document carries these values), a list of classes
                r = rows_q[b]
                if isinstance(c, list):
                    r = r[np.isin(corpus._classes.ids[r], np.asarray(c, np.int64))] if c else r[:0]
                elif c != -1:
                    r = r[corpus._classes.ids[r] == c]
                rows_q[b], dicts[b] = r, None
        return rows_q, dicts

    def _host_mask(self, spec, rows: Optional[np.ndarray]):
        """The host walk's arguments for one query: (filter_dict, rows).  A dict stays the walk's own equality test; a set filter
        becomes the rows it matches (with `rows`: those of them)."""
        if not isinstance(spec, _SetFilter):
            return spec, rows
        allowed = self._corpus_state.rows_matching(spec)
        return None, allowed if rows is None else np.intersect1d(rows, allowed, assume_unique=True)

    def _topk_planned(self, tok: Sequence[np.ndarray], plan: List[Any]):
        """One key-set group after corpus.plan: queries whose filter matches no row get nothing (no scan); a group without a set of two
        or more classes is today's class-column call, any other erh_bm25_topk_sets."""
        B, k = len(plan), self._similarity_top_k
        if any(isinstance(c, list) and len(c) > 1 for c in plan):
            qi, qt = queries_to_csr(tok)
            return self.engine.bm25_topk_sets(qi, qt, k, [None if c == -1 else (c if isinstance(c, list) else [c]) for c in plan],
                                              slot=self._slot)
        ids, sc, ln = np.full((B, k), -1, np.int32), np.zeros((B, k), np.float64), np.zeros(B, np.int32)
        live = [b for b in range(B) if not isinstance(plan[b], list)]
        if live:
            col = np.asarray([plan[b] for b in live], np.int16)
            qi, qt = queries_to_csr([tok[b] for b in live])
            ids[live], sc[live], ln[live] = self.engine.bm25_topk(qi, qt, k, slot=self._slot, filter_dir=col if np.any(col >= 0) else None)
        return ids, sc, ln

    def retrieve_batch(self, queries: Sequence[str], filter_dicts=_UNSET, rows=None, filters=_UNSET,
                       exclude=None) -> List[List[NodeWithScore]]:
        """get_scores + filter for a whole batch, fused on the GPU (no score vector leaves the chip).  `filter_dicts`
        (default: the `filter_dict` attribute, for every query) may be a list parallel to `queries`: one dict / None each.
        `filters` (default: the `filters` attribute): a Qdrant-style Filter -- MatchValue / MatchAny / MatchExcept / Range, must / should /
        must_not with nesting, compiled like the dense route's (unsupported elements raise TypeError before any engine call) -- or a list
        of them parallel to `queries`.  A query with a filter_dict and a filter sees the rows that pass BOTH.  Every class allowed: the
        unfiltered call; one class: the class-column call; none: an empty list without a call; two or more: erh_bm25_topk_sets.
        `rows`: restrict queries to explicit node positions -- one id array for every query, or a list parallel to the queries whose
        entries are an id array or None (HipVectorStore.query_batch's argument, normalised the same way).  Such a query ranks exactly
        those rows by the corpus index's BM25 (erh_bm25_topk_rows; with a filter as well: the rows that also pass it), the others
        run as without the argument, and the two parts are scattered into one result.
        `exclude`: QdrantRetriever.retrieve_batch's argument -- what a query must NOT return (positions, node ids, nodes or NodeWithScore;
        one entry for every query or one each); must_not: [HasIdCondition] in `filters` is the same thing, must: [HasIdCondition] a rows
        list.  Such a query takes erh_bm25_topk_excl when k + its exclusions fit the call's depth, else the complement as a rows list."""
        B = len(queries)
        if B == 0:
            return []
        dicts = _per_query(self.filter_dict if filter_dicts is _UNSET else filter_dicts, B, lambda v: dict(v) if v else None)
        fl, rows, excl_q = _lift_id_conditions(self.filters if filters is _UNSET else filters, rows, exclude, B, len(self._nodes),
                                               lambda e: _id_positions(self, self._nodes, e, "retriever"))
        if fl is not None:
            dicts = [_both(d, f) for d, f in zip(dicts, _per_query(fl, B, _spec_cache()))]
        tok = [self._query_ids(q) for q in queries]
        k = self._similarity_top_k
        rows_q, dicts = self._resolve_rows(dicts, rows, B)
        drop: List[int] = []
        if excl_q is not None and any(e.size for e in excl_q):
            in_range = 1 <= k <= BM25_DEVICE_MAX_K
            for b in range(B):
                if rows_q[b] is not None:
                    rows_q[b] = _without(rows_q[b], excl_q[b])
                elif in_range and plan_exclusion(k, excl_q[b].size, BM25_DEVICE_MAX_K) == "drop":
                    drop.append(b)
                elif excl_q[b].size:
                    rows_q[b], dicts[b] = _without(_allowed_rows(self._corpus_state, dicts[b]), excl_q[b]), None
        if not 1 <= k <= BM25_DEVICE_MAX_K:
            # outside the fused kernels' range (erh_bm25_topk: 1 <= k <= 1024) the reference's answer is still defined: the
            # score vector plus the host filter (restricted to the rows; a set filter as the rows it matches) give it exactly
            masks = [self._host_mask(d, r) for d, r in zip(dicts, rows_q)]
            return [self._filter_one(self._cast(self.engine.bm25_scores(t, slot=self._slot)), fd, k, rows=keep)
                    for t, (fd, keep) in zip(tok, masks)]
        out: List[List[NodeWithScore]] = [[] for _ in range(B)]
        for g in _by_key_set([dicts[b] for b in drop]):
            g = [drop[j] for j in g]
            qi, qt = queries_to_csr([tok[b] for b in g])
            ids, sc, ln = self.engine.bm25_topk_excl(qi, qt, k, [excl_q[b] for b in g],
                                                     sets=_plan_sets(self._corpus_state.plan([dicts[b] for b in g])), slot=self._slot)
            for j, b in enumerate(g):
                out[b] = [NodeWithScore(node=self._nodes[i], score=float(s)) for i, s in zip(ids[j, :ln[j]], sc[j, :ln[j]])]
        rest = [b for b in range(B) if rows_q[b] is None and b not in drop]
        for g in _by_key_set([dicts[b] for b in rest]):
            g = [rest[j] for j in g]
            if any(isinstance(dicts[b], _SetFilter) for b in g):
                ids, sc, ln = self._topk_planned([tok[b] for b in g], self._corpus_state.plan([dicts[b] for b in g]))
            else:
                qi, qt = queries_to_csr([tok[b] for b in g])
                ids, sc, ln = self.engine.bm25_topk(qi, qt, self._similarity_top_k, slot=self._slot,
                                                    filter_dir=self._corpus_state.filter_column([dicts[b] for b in g]))
            for j, b in enumerate(g):
                out[b] = [NodeWithScore(node=self._nodes[i], score=float(s)) for i, s in zip(ids[j, :ln[j]], sc[j, :ln[j]])]
        with_rows = [b for b in range(B) if rows_q[b] is not None]
        if with_rows:
            lists, list_of = _rows_lists([rows_q[b] for b in with_rows])
            qi, qt = queries_to_csr([tok[b] for b in with_rows])
            ids, sc, ln = self.engine.bm25_topk_rows(qi, qt, k, lists, list_of=list_of, slot=self._slot)
            for j, b in enumerate(with_rows):
                out[b] = [NodeWithScore(node=self._nodes[i], score=float(s)) for i, s in zip(ids[j, :ln[j]], sc[j, :ln[j]])]
        return out

    def score_nodes(self, query: str, nodes_or_ids, top_k: Optional[int] = None) -> List[NodeWithScore]:
        """The given nodes -- positions in the node list, or node objects of it (NodeWithScore included) -- and nothing else, ranked by
        the CORPUS index's BM25: the sparse twin of QdrantRetriever.score_nodes.  Every node gets its exact score on the device (one
        call, the nodes in lists of at most 1024, the call's limit on k); only nodes with a score > 0 are returned, as everywhere on
        this route; (score desc, position asc); `top_k` cuts the result.
        Not get_scores(query, docs): that one builds a throw-away index over the given strings, so its idf and avgdl are THEIRS and a
        score there depends on which other strings were passed; here idf, avgdl and document lengths are the corpus's, and a node's
        score is the one retrieve() would report for it."""
        ids = _node_positions(self, self._nodes, nodes_or_ids, "retriever")
        if ids.size == 0:
            return []
        chunks = [ids[i:i + BM25_DEVICE_MAX_K] for i in range(0, ids.size, BM25_DEVICE_MAX_K)]
        qi, qt = queries_to_csr([self._query_ids(query)] * len(chunks))
        got, sc, ln = self.engine.bm25_topk_rows(qi, qt, len(chunks[0]), chunks, slot=self._slot)
        got = np.concatenate([got[j, :ln[j]] for j in range(len(chunks))])
        sc = np.concatenate([sc[j, :ln[j]] for j in range(len(chunks))])
        order = np.lexsort((got, -sc))                     # (one chunk: already in this order)
        if top_k is not None:
            order = order[:max(int(top_k), 0)]
        return [NodeWithScore(node=self._nodes[int(got[i])], score=float(sc[i])) for i in order]


_SCRATCH_LOCK = threading.Lock()
_FUSION_ENGINE: Optional[RetrievalEngine] = None
_FUSION_LOCK = threading.Lock()


def _fusion_engine() -> RetrievalEngine:
    global _FUSION_ENGINE
    if _FUSION_ENGINE is None:
        _FUSION_ENGINE = RetrievalEngine()
    return _FUSION_ENGINE


def _lists_to_device_form(lists):
    """Flatten lists of NodeWithScore into local item ids + content ids for the fusion kernels."""
    items, cid, key = [], [], {}
    per_list = []
    for lst in lists:
        ids = []
        for it in lst:
            ids.append(len(items))
            cid.append(key.setdefault(it.get_content(), len(key)))
            items.append(it)
        per_list.append(ids)
    return items, np.asarray(cid, np.int32), per_list


class HybridRetriever(_RetrieverBase):
    def __init__(self, dense_retriever: QdrantRetriever, sparse_retriever: BM25Retriever, retrieval_type: int = 1,
                 topk: int = 256):
        self.dense_retriever = dense_retriever
        self.sparse_retriever = sparse_retriever
        self.retrieval_type = retrieval_type     # 1: dense only  2: sparse only  3: hybrid (RRF)
        self.filters = None
        self.filter_dict = None
        self.topk = topk
        self._init_base()

    # -- classmethods over already-retrieved lists (ref retrievers.py:239-274) ----------------------------
    # The pipeline calls them once per query on a few hundred NodeWithScore objects it already holds on the host
    # (pipeline.py:362, 408: 192 + 6 or 192 + 288 items).  A kernel launch plus six PCIe stagings for that is slower than
    # the reference's own loop, so lists of up to `fusion_device_min` items are merged right here on the objects (any
    # number of lists, as the reference accepts); the library's fusion kernels (erh_rrf / erh_fusion, and the fused
    # erh_hybrid_topk that `aretrieve` runs) take over for larger inputs and for everything that is already on the device.
    fusion_device_min = 512          # (and at most 2048 items: the kernels' LDS budget)

    @staticmethod
    def _fuse_host(lists, rrf: bool, K: int, topk: int):
        if not rrf:                                  # first occurrence of a content wins, raw scores, stable sort
            seen, merged = set(), []
            for lst in lists:
                for node in lst:
                    c = node.get_content()
                    if c not in seen:
                        merged.append(node)
                        seen.add(c)
            merged.sort(key=lambda node: node.score, reverse=True)
            return merged[:min(len(merged), topk)]
        score, last = {}, {}                         # dict order = first appearance; the LAST node of a content is returned
        for lst in lists:
            for rank, item in enumerate(lst, 1):
                c = item.get_content()
                last[c] = item
                score[c] = score.get(c, 0.0) + 1 / (rank + K)
        out = []
        for c, sc in sorted(score.items(), key=lambda kv: kv[1], reverse=True):
            node = last[c]
            node.score = sc                          # the reference overwrites the node's score with the RRF score
            out.append(node)
        return out[:min(topk, len(out))]

    @classmethod
    def _fuse(cls, lists, rrf: bool, K: int, topk: int):
        lists = [list(x) for x in lists]
        n_items = sum(len(x) for x in lists)
        if n_items <= cls.fusion_device_min or n_items > FUSE_MAX_ITEMS or len(lists) > 2 or topk <= 0:
            return cls._fuse_host(lists, rrf, K, topk)       # (topk <= 0: the reference slices [:0] / [:topk])
        if len(lists) == 1:
            lists.append([])
        items, cid, per_list = _lists_to_device_form(lists)
        if not items:
            return []
        # the kernel is asked for every fused row (n_items bounds the distinct contents): the reference writes the RRF score
        # into EVERY fused node, those cut by topk included, and slices afterwards
        rows = n_items
        da, db = max(len(per_list[0]), 1), max(len(per_list[1]), 1)
        ia = np.full((1, da), -1, np.int32)
        ib = np.full((1, db), -1, np.int32)
        ia[0, :len(per_list[0])] = per_list[0]
        ib[0, :len(per_list[1])] = per_list[1]
        la = np.asarray([len(per_list[0])], np.int32)
        lb = np.asarray([len(per_list[1])], np.int32)
        with _FUSION_LOCK:                       # the classmethods share one small handle (item ids are list-local)
            eng = _fusion_engine()
            eng.set_doc_meta(len(items), cid, None)
            if rrf:
                ids, sc, ln = eng.rrf(ia, la, ib, lb, K=K, topk=rows)
            else:
                sa = np.zeros((1, da), np.float64)
                sb = np.zeros((1, db), np.float64)
                sa[0, :la[0]] = [items[i].score for i in per_list[0]]
                sb[0, :lb[0]] = [items[i].score for i in per_list[1]]
                ids, sc, ln = eng.fusion(ia, sa, la, ib, sb, lb, topk=rows)
        out = []
        for i, s in zip(ids[0, :ln[0]], sc[0, :ln[0]]):
            node = items[i]
            if rrf:
                node.score = float(s)        # the reference overwrites the node's score with the RRF score
            out.append(node)
        return out[:topk]

    @classmethod
    def fusion(cls, list_of_list_ranks_system, topk: int = 256):
        return cls._fuse(list_of_list_ranks_system, rrf=False, K=0, topk=topk)

    @classmethod
    def reciprocal_rank_fusion(cls, list_of_list_ranks_system, K: int = 60, topk: int = 256):
        return cls._fuse(list_of_list_ranks_system, rrf=True, K=K, topk=topk)

    # -- routes ---------------------------------------------------------------------------------------------
    def _fused_possible(self) -> bool:
        vs = getattr(self.dense_retriever, "_vector_store", None)
        return (isinstance(vs, HipVectorStore) and vs.engine is self.sparse_retriever.engine
                and len(vs.nodes) == len(self.sparse_retriever._nodes))

    def _fused_sizes(self) -> bool:
        """topk / k_sparse / k_dense within what erh_hybrid_topk accepts."""
        ks, kd = self.sparse_retriever._similarity_top_k, self.dense_retriever._similarity_top_k
        return self.topk >= 1 and 1 <= ks <= BM25_DEVICE_MAX_K and 1 <= kd <= DENSE_MAX_K and ks + kd <= FUSE_MAX_ITEMS

    def _retrieve(self, query_bundle: QueryBundle) -> List[NodeWithScore]:
        """The reference's sync path (retrievers.py:293-305, marked unmaintained there): both routes with whatever
        filters the child retrievers currently hold, sparse list then dense list, de-duplicated by node_id; no
        route selection, no RRF, no filter push-down.  The pipeline calls `aretrieve`."""
        sparse_nodes = self.sparse_retriever.retrieve(query_bundle)
        dense_nodes = self.dense_retriever.retrieve(query_bundle)
        all_nodes, node_ids = [], set()
        for n in sparse_nodes + dense_nodes:
            if n.node.node_id not in node_ids:
                all_nodes.append(n)
                node_ids.add(n.node.node_id)
        return all_nodes

    async def _aretrieve(self, query_bundle: QueryBundle) -> List[NodeWithScore]:
        """Route selection + filter push-down + RRF (retrievers.py:276-291)."""
        return self.retrieve_batch([query_bundle.query_str])[0]

    def retrieve_batch(self, queries: Sequence[str], filter_dicts=_UNSET, filters=_UNSET, rows=None,
                       sparse_rows=None, sparse_filters=_UNSET, exclude=None) -> List[List[NodeWithScore]]:
        """`_aretrieve` for a batch of query strings.  Without the keyword arguments the `filter_dict` / `filters`
        attributes apply to every query and are pushed into the child retrievers as the reference does
        (retrievers.py:278,283).  `filter_dicts` (sparse route) / `filters` (dense route) may instead be lists parallel to
        `queries` -- the reference's evaluation loop changes both before every question (pipeline.py:301-312,331-341), so a
        batch of its questions needs one filter per query; the child retrievers' attributes are left alone then.
        `rows` restricts the DENSE route (QdrantRetriever.retrieve_batch's argument); the sparse route keeps its filter_dict.
        `sparse_rows` restricts the SPARSE route (BM25Retriever.retrieve_batch's `rows`); the same object passed as both holds the
        fused call to one id set: RRF then runs on two lists drawn from the same population.
        `sparse_filters` (not given: the sparse route gets its filter_dict only, as in the reference) hands the SPARSE route a Qdrant-style
        Filter as well (BM25Retriever.retrieve_batch's `filters`; one, or a list parallel to `queries`); the same object passed as
        `filters` and `sparse_filters` holds both routes to one population -- erh_bm25_topk_sets and erh_dense_topk_sets into device
        buffers, then the RRF kernel.
        `exclude` (the child retrievers' argument; must_not: [HasIdCondition] in `filters` / `sparse_filters` adds to it, on its own
        route) goes to BOTH routes, so the two lists are ranked over one population: erh_bm25_topk_excl and erh_dense_topk_excl into
        device buffers, then the RRF kernel; where that composition does not apply, the routes on their own + RRF."""
        sp, de = self.sparse_retriever, self.dense_retriever
        B = len(queries)
        if B == 0:
            return []
        fs = self.filter_dict if filter_dicts is _UNSET else filter_dicts
        fdn = self.filters if filters is _UNSET else filters
        if exclude is not None or _has_id_conditions(fdn) or (sparse_filters is not _UNSET and _has_id_conditions(sparse_filters)):
            return self._retrieve_excluding(queries, fs, fdn, rows, sparse_rows, sparse_filters, exclude,
                                            filter_dicts is _UNSET, filters is _UNSET)
        s_kw = {} if sparse_rows is None else {"rows": sparse_rows}
        if sparse_filters is not _UNSET:
            s_kw["filters"] = sparse_filters
        if self.retrieval_type != 1:
            if filter_dicts is _UNSET:
                sp.filter_dict = self.filter_dict
            if self.retrieval_type == 2:
                return sp.retrieve_batch(queries, filter_dicts=fs, **s_kw)
        if self.retrieval_type != 2:
            if filters is _UNSET:
                de.filters = self.filters
            if self.retrieval_type == 1:
                return de.retrieve_batch(queries, filters=fdn, rows=rows)
        # filter_dict restricts the sparse route only, filters the dense route only (retrievers.py:278,283)
        d_sparse = _per_query(fs, B, lambda v: dict(v) if v else None)
        spec = _spec_cache()                           # (one cache: the same object on both routes compiles once)
        d_dense = _per_query(fdn, B, spec)
        if sparse_filters is not _UNSET and sparse_filters is not None:
            d_sparse = [_both(d, f) for d, f in zip(d_sparse, _per_query(sparse_filters, B, spec))]
        key_sets = {_spec_keys(fd) for fd in d_sparse + d_dense if _spec_keys(fd)}
        s_sets = any(isinstance(fd, _SetFilter) for fd in d_sparse)
        # a sparse filter over more distinct values than a class column numbers runs through the sparse route's own rows entry
        s_many = self._fused_possible() and any(
            _spec_keys(fd) and sp._corpus_state.too_many_values(_spec_keys(fd)) for fd in d_sparse if fd)
        if not self._fused_possible() or len(key_sets) > 1 or not self._fused_sizes() or (s_many and sparse_rows is None):
            # (outside erh_hybrid_topk's sizes the routes run on their own: each one falls back or names its limit)
            sparse, dense = sp.retrieve_batch(queries, filter_dicts=fs, **s_kw), de.retrieve_batch(queries, filters=fdn, rows=rows)
            return [self.reciprocal_rank_fusion([s, d], topk=self.topk) for s, d in zip(sparse, dense)]
        vs = de._vector_store
        if sparse_rows is not None:
            s_rows_q, _ = sp._resolve_rows(d_sparse, sparse_rows, B)
            rows_q, _ = vs._resolve_rows(d_dense, rows, B, _lib.ERH_DENSE_EXACT)
            if all(r is not None for r in s_rows_q) and all(r is not None for r in rows_q):
                return self._retrieve_rows(queries, d_sparse, rows_q, s_rows_q)
            # any mixture of rows and non-rows queries on either route: the routes on their own + RRF
            sparse, dense = sp.retrieve_batch(queries, filter_dicts=fs, **s_kw), de.retrieve_batch(queries, filters=fdn, rows=rows)
            return [self.reciprocal_rank_fusion([s, d], topk=self.topk) for s, d in zip(sparse, dense)]
        if rows is not None or any(sp and _spec_keys(sp) and vs.corpus.too_many_values(_spec_keys(sp)) for sp in d_dense):
            rows_q, _ = vs._resolve_rows(d_dense, rows, B, _lib.ERH_DENSE_EXACT)
            if s_sets or any(r is None for r in rows_q):
                # a batch that mixes rows and non-rows dense queries, or a set filter on the sparse route beside dense rows: the routes
                # on their own + RRF
                sparse, dense = sp.retrieve_batch(queries, filter_dicts=fs, **s_kw), de.retrieve_batch(queries, filters=fdn, rows=rows)
                return [self.reciprocal_rank_fusion([s, d], topk=self.topk) for s, d in zip(sparse, dense)]
            return self._retrieve_rows(queries, d_sparse, rows_q)
        if s_sets or any(isinstance(fd, _SetFilter) for fd in d_dense):
            return self._retrieve_sets(queries, d_sparse, d_dense)
        # both routes share one engine: BM25 -> dense -> RRF([sparse, dense]) in a single device pipeline, one class column
        # per route over the shared key set (a query's two filters may still differ, or one of them be absent)
        cstate = sp._corpus_state
        filt_s, filt_d = cstate.filter_column(d_sparse), cstate.filter_column(d_dense)
        qi, qt = queries_to_csr([sp._query_ids(q) for q in queries])
        embs = _unit_f16(np.asarray([de._embed_model.get_query_embedding(q) for q in queries], dtype=np.float32))
        ids, sc, ln = sp.engine.hybrid_topk(embs, qi, qt, k_dense=de._similarity_top_k,
                                            k_sparse=sp._similarity_top_k, K=60, topk=self.topk,
                                            filter_dir=filt_s, filter_dense=filt_d, slot=sp._slot)
        nodes = sp._nodes
        return [[NodeWithScore(node=nodes[i], score=float(s)) for i, s in zip(ids[b, :ln[b]], sc[b, :ln[b]])]
                for b in range(B)]

    def _retrieve_excluding(self, queries: Sequence[str], fs, fdn, rows, sparse_rows, sparse_filters, exclude,
                            push_filter_dict: bool, push_filters: bool) -> List[List[NodeWithScore]]:
        """retrieve_batch with `exclude`.  retrieval_type 3 on one engine, one key set, no row lists and every exclusion within both
        routes' depths: erh_bm25_topk_excl and erh_dense_topk_excl into device buffers (the dense entry checks its inner call itself),
        the RRF kernel over the two device lists, one synchronisation.  Anything else: the child retrievers with the exclusion + RRF."""
        sp, de = self.sparse_retriever, self.dense_retriever
        B = len(queries)
        excl_q = _per_query_exclude(exclude, B, lambda e: _id_positions(sp, sp._nodes, e, "retriever"))
        s_kw: Dict[str, Any] = {} if sparse_rows is None else {"rows": sparse_rows}
        if sparse_filters is not _UNSET:
            s_kw["filters"] = sparse_filters
        x_kw: Dict[str, Any] = {} if excl_q is None else {"exclude": excl_q}
        if self.retrieval_type != 1 and push_filter_dict:
            sp.filter_dict = self.filter_dict
        if self.retrieval_type != 2 and push_filters:
            de.filters = self.filters
        if self.retrieval_type == 2:
            return sp.retrieve_batch(queries, filter_dicts=fs, **x_kw, **s_kw)
        if self.retrieval_type == 1:
            return de.retrieve_batch(queries, filters=fdn, rows=rows, **x_kw)

        def on_their_own():
            sparse = sp.retrieve_batch(queries, filter_dicts=fs, **x_kw, **s_kw)
            dense = de.retrieve_batch(queries, filters=fdn, rows=rows, **x_kw)
            return [self.reciprocal_rank_fusion([s, d], topk=self.topk) for s, d in zip(sparse, dense)]
        if not self._fused_possible() or not self._fused_sizes() or rows is not None or sparse_rows is not None:
            return on_their_own()
        resolve = lambda e: _id_positions(sp, sp._nodes, e, "retriever")
        n = len(sp._nodes)
        fdn_l, d_rows, excl_d = _lift_id_conditions(fdn, None, excl_q, B, n, resolve)
        sfl, s_rows, excl_s = _lift_id_conditions(None if sparse_filters is _UNSET else sparse_filters, None, excl_q, B, n, resolve)
        if d_rows is not None or s_rows is not None:
            return on_their_own()
        none = [np.zeros(0, np.int64)] * B
        excl_s, excl_d = excl_s or none, excl_d or none
        ks, kd = sp._similarity_top_k, de._similarity_top_k
        if (max(e.size for e in excl_s) + ks > BM25_DEVICE_MAX_K) or (max(e.size for e in excl_d) + kd > DENSE_MAX_K):
            return on_their_own()
        spec = _spec_cache()
        d_sparse = _per_query(fs, B, lambda v: dict(v) if v else None)
        d_dense = _per_query(fdn_l, B, spec)
        if sfl is not None:
            d_sparse = [_both(d, f) for d, f in zip(d_sparse, _per_query(sfl, B, spec))]
        key_sets = {_spec_keys(fd) for fd in d_sparse + d_dense if _spec_keys(fd)}
        cstate = sp._corpus_state
        if len(key_sets) > 1 or any(cstate.too_many_values(ks_) for ks_ in key_sets):
            return on_their_own()
        eng = sp.engine
        sets_s, sets_d = _plan_sets(cstate.plan(d_sparse)), _plan_sets(cstate.plan(d_dense))
        qi, qt = queries_to_csr([sp._query_ids(q) for q in queries])
        embs = _unit_f16(np.asarray([de._embed_model.get_query_embedding(q) for q in queries], dtype=np.float32))
        sids, _, sln = eng.bm25_topk_excl(qi, qt, ks, excl_s, sets=sets_s, device_out=True, slot=sp._slot)
        dids, _, dln = eng.dense_topk_excl(embs, kd, excl_d, sets=sets_d, device_out=True)
        fids, fsc, fln = eng.rrf_device(sids, sln, dids, dln, K=60, topk=self.topk)
        eng.sync()
        ids, sc, ln = fids.cpu().numpy(), fsc.cpu().numpy(), fln.cpu().numpy()
        nodes = sp._nodes
        return [[NodeWithScore(node=nodes[i], score=float(s)) for i, s in zip(ids[b, :ln[b]], sc[b, :ln[b]])]
                for b in range(B)]

    def _retrieve_sets(self, queries: Sequence[str], d_sparse, d_dense) -> List[List[NodeWithScore]]:
        """retrieval_type 3 with a set-valued filter on either route: every step on the device, no host round trip between them -- BM25
        top-k (class column of filter_dict; with a set filter on the sparse route, `sparse_filters`: erh_bm25_topk_sets) and
        erh_dense_topk_sets into device buffers, erh_dense_check (sub-queries answered by the exhaustive path merged again), then the
        RRF kernel over the two device lists."""
        sp, de = self.sparse_retriever, self.dense_retriever
        eng, cstate = sp.engine, sp._corpus_state
        B = len(queries)
        s_sets = any(isinstance(fd, _SetFilter) for fd in d_sparse)
        if s_sets:
            plan_s = cstate.plan(d_sparse)
        else:
            filt_s = cstate.filter_column(d_sparse)
        plan = cstate.plan(d_dense)                    # (same key set as the sparse route's: the caller checked; the column stays put)
        qi, qt = queries_to_csr([sp._query_ids(q) for q in queries])
        embs = _unit_f16(np.asarray([de._embed_model.get_query_embedding(q) for q in queries], dtype=np.float32))
        if s_sets:
            sids, _, sln = eng.bm25_topk_sets(qi, qt, sp._similarity_top_k,
                                              [None if c == -1 else (c if isinstance(c, list) else [c]) for c in plan_s],
                                              device_out=True, slot=sp._slot)
        else:
            sids, _, sln = eng.bm25_topk(qi, qt, sp._similarity_top_k, filter_dir=filt_s, device_out=True, slot=sp._slot)
        dids, _, dln = eng.dense_topk_sets(embs, de._similarity_top_k,
                                           [None if c == -1 else (c if isinstance(c, list) else [c]) for c in plan], device_out=True)
        eng.dense_check()
        fids, fsc, fln = eng.rrf_device(sids, sln, dids, dln, K=60, topk=self.topk)
        eng.sync()
        ids, sc, ln = fids.cpu().numpy(), fsc.cpu().numpy(), fln.cpu().numpy()
        nodes = sp._nodes
        return [[NodeWithScore(node=nodes[i], score=float(s)) for i, s in zip(ids[b, :ln[b]], sc[b, :ln[b]])]
                for b in range(B)]

    def _retrieve_rows(self, queries: Sequence[str], d_sparse, rows_q, s_rows_q=None) -> List[List[NodeWithScore]]:
        """retrieval_type 3 with explicit rows on the dense side, every step on the device: BM25 top-k (class column of filter_dict; with
        `s_rows_q`, the sparse route's own row lists with its filter already applied: erh_bm25_topk_rows) and erh_dense_topk_rows into
        device buffers, the RRF kernel over the two device lists, one synchronisation (the rows entries leave nothing for
        erh_dense_check)."""
        sp, de = self.sparse_retriever, self.dense_retriever
        eng, cstate = sp.engine, sp._corpus_state
        B = len(queries)
        lists, list_of = de._vector_store._rows_lists(rows_q)
        qi, qt = queries_to_csr([sp._query_ids(q) for q in queries])
        embs = _unit_f16(np.asarray([de._embed_model.get_query_embedding(q) for q in queries], dtype=np.float32))
        if s_rows_q is None:
            filt_s = cstate.filter_column(d_sparse)
            sids, _, sln = eng.bm25_topk(qi, qt, sp._similarity_top_k, filter_dir=filt_s, device_out=True, slot=sp._slot)
        else:
            s_lists, s_list_of = _rows_lists(s_rows_q)
            sids, _, sln = eng.bm25_topk_rows(qi, qt, sp._similarity_top_k, s_lists, list_of=s_list_of, device_out=True, slot=sp._slot)
        dids, _, dln = eng.dense_topk_rows(embs, de._similarity_top_k, lists, list_of=list_of, device_out=True)
        fids, fsc, fln = eng.rrf_device(sids, sln, dids, dln, K=60, topk=self.topk)
        eng.sync()
        ids, sc, ln = fids.cpu().numpy(), fsc.cpu().numpy(), fln.cpu().numpy()
        nodes = sp._nodes
        return [[NodeWithScore(node=nodes[i], score=float(s)) for i, s in zip(ids[b, :ln[b]], sc[b, :ln[b]])]
                for b in range(B)]
