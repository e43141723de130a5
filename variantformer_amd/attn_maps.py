"""Attention maps of the registry tokens: the sink the gene layers write their softmax probabilities into -- the cross
attention over the gene's cCREs (`maps`) and, with gene_body=True, the self attention over the token's own sequence, the
registry token and the gene-body chunks behind it (`gene_maps`).

Held in a context variable like runtime.Switches (no module globals; `with` blocks nest and restore; a thread starts
without a capture), so a capture requested around one model's forward never reaches another thread's.  Off unless a
`capture(...)` block is open: the layer stack then makes not one launch or allocation more than without this module.

    with attn_maps.capture(layers=(0, 24), per_head=False) as cap:
        model.forward_prepared(pb)            # or predict_launch / predict_finish
    cap.maps                                  # fp32 [len(layers), sum T (* H), max_cre], row r = row r of `emb`
    cap.gene_maps                             # gene_body=True: fp32 [len(layers), sum T (* H), max_gene], column 0 = the token itself
    cap.contrib                               # contributions=True: shaped like cap.maps; || sum_h P_h Wo_h v_j ||, what the token RECEIVED
    cap.gene_contrib                          # gene_contributions=True: shaped like cap.gene_maps; the same norms for the self attention

Who calls what: the model's forward `begin`s the capture with the batch's selected rows (the registry-token rows, the
only rows the expression head reads); modulator_forward_packed wraps every GENE layer in `cap.layer(i, ...)`; MHA.attend's
cross branch asks `running()` and, inside a requested gene layer only, hands q and K (with contributions: also V and the
module's Gram matrix of out_proj, MHA.contrib_gram) to `record`; MHA.attend_qkv and the last
layer's forward_packed_rows hand the self attention's q and K (and V and the packed out_proj weight, which only the gene-body
contributions read) to `record_self` at the same places.  The CRE layers run
outside any `layer(...)` block and are never captured.  DESIGN.md section 5b.
"""
from __future__ import annotations

import contextvars

import torch

from . import ops

_CAP: contextvars.ContextVar = contextvars.ContextVar("vf_attn_capture", default=None)


class Capture:
    def __init__(self, layers, per_head: bool = False, gene_body: bool = False, contributions: bool = False,
                 gene_contributions: bool = False):
        self.layers = tuple(int(i) for i in layers)     # distinct gene-layer indices, in the order of the first axis of `maps`
        if not self.layers or len(set(self.layers)) != len(self.layers):
            raise ValueError(f"attention maps: a capture needs distinct gene layers, got {list(self.layers)}")
        self.per_head = bool(per_head)
        self.gene_body = bool(gene_body)
        self.contributions = bool(contributions)
        self.contrib = None       # contributions: fp32, shaped like `maps`: the value-weighted norms of the most recent forward
        self._scratch = None      # contributions: (gram fp32 [keys, H, H], per-head P fp32 [R * H, max_k] | None), one per forward
        self.gene_contributions = bool(gene_contributions)
        self.gene_contrib = None  # gene_contributions: fp32, shaped like `gene_maps`: the self attention's value-weighted norms
        self._self_scratch = None  # gene_contributions: per-head P fp32 [R * H, max_gene] when the gene map itself is not it
        self.maps = None          # fp32 [len(layers), R or R * H, max_k] of the most recent forward
        self.gene_maps = None     # gene_body: fp32 [len(layers), R or R * H, max_gene] of the most recent forward
        self.shape = None         # the forward's (tissues, cCREs, chunks) per gene: how the rows and columns split (host lists)
        self._self = None         # (cu_rows int32 [n_seq + 1], cu_k int32 [n_seq + 1], max_k): the self-attention grouping
        self.n_rows = 0
        self._rows = None         # (q_rows int64 [R], cu_rows int32 [n_seq + 1], max_rows, cu_k int32 [n_seq + 1], max_k)
        self._running = None      # (slot in `layers`, compact: the query buffer holds exactly the selected rows)

    def begin(self, q_rows, cu_rows, max_rows: int, cu_k, max_k: int, gene_self=None, shape=None) -> None:
        """A forward starts: its selected rows (row q_rows[r] of the gene layers' query buffer, grouped per key sequence by
        cu_rows) and keys.  gene_self = (cu_rows, cu_k, max_k): the same rows grouped per SELF-attention sequence and those
        sequences' keys (every selected row sits at position 0 of its sequence).  The buffers are the forward's own: a second
        forward under the same capture (the LayerNorm-fold recomputation) starts afresh and the maps are then its result."""
        self._rows = (q_rows, cu_rows, int(max_rows), cu_k, int(max_k))
        self._self = None if gene_self is None else (gene_self[0], gene_self[1], int(gene_self[2]))
        self.n_rows = int(q_rows.numel())
        self.shape = shape
        self.maps = None
        self.gene_maps = None
        self.contrib = None
        self._scratch = None
        self.gene_contrib = None
        self._self_scratch = None

    def layer(self, i: int, compact: bool = False):
        """with cap.layer(i): gene layer i is running.  compact: its cross attention's query buffer already is the selected rows,
        in order (the last layer's registry-rows form)."""
        return _Layer(self, i, compact)

    def record(self, q, k, n_heads: int, head_dim: int, family: str = "", v=None, s_gram=None) -> None:
        """The running gene layer's cross attention: q / k its 16-bit query and key operands.  With contributions also v, the
        value operand the attention kernel reads, and s_gram, fp32 [H, H, dh, dh] of the layer's out_proj (MHA.contrib_gram):
        the per-head P (the map itself with per_head, else a second call into a scratch; the head-mean map keeps its call and
        bits) feeds ops.attn_contrib.  Scratch and the keys' Gram buffer are made once per forward and shared by the layers."""
        slot, compact = self._running
        q_rows, cu_rows, max_rows, cu_k, max_k = self._rows
        n_out = self.n_rows * (n_heads if self.per_head else 1)
        if self.maps is None:
            self.maps = torch.empty((len(self.layers), n_out, max_k), dtype=torch.float32, device=q.device)
        if compact:
            assert q.shape[0] == self.n_rows
        ops.attn_probs(q, k, cu_rows, cu_k, max_rows, max_k, n_heads, head_dim, q_rows=None if compact else q_rows,
                       q_log2=True, per_head=self.per_head, out=self.maps[slot], family=family + "_maps")
        if not self.contributions:
            return
        if self.contrib is None:
            self.contrib = torch.empty((len(self.layers), n_out, max_k), dtype=torch.float32, device=q.device)
            self._scratch = (torch.empty((k.shape[0], n_heads, n_heads), dtype=torch.float32, device=q.device),
                             None if self.per_head else torch.empty((self.n_rows * n_heads, max_k), dtype=torch.float32, device=q.device))
        gram, probs = self._scratch
        if self.per_head:
            probs = self.maps[slot]
        else:
            ops.attn_probs(q, k, cu_rows, cu_k, max_rows, max_k, n_heads, head_dim, q_rows=None if compact else q_rows,
                           q_log2=True, per_head=True, out=probs, family=family + "_contrib")
        ops.attn_contrib(v, s_gram, probs, cu_rows, cu_k, max_rows, max_k, n_heads, head_dim, gram=gram, out=self.contrib[slot],
                         per_head=self.per_head, family=family + "_contrib")

    def record_self(self, q, k, n_heads: int, head_dim: int, slopes=None, rows=None, family: str = "", v=None, wo=None) -> None:
        """The running gene layer's SELF attention: q / k its 16-bit query and key operands, slopes its ALiBi slopes (None: a
        model built without), rows int64 [tokens]: q and k (and v) are a table of distinct projected rows and token t's row is
        rows[t] (the first gene layer).  The selected rows are registry tokens: position 0 of their sequences, one per
        sequence.  v / wo: the value operand the attention kernel reads and the 16-bit out_proj weight the GEMM multiplies;
        only gene_contributions reads them: the per-head P (the gene map itself with per_head and gene_body, else a second
        call into a scratch; the head-mean gene map keeps its call and bits) feeds ops.attn_contrib_self.  The scratch and
        gene_contrib are made once per forward and shared by the layers."""
        slot, compact = self._running
        cu_rows, cu_k, max_k = self._self
        q_rows = None if compact else self._rows[0]
        n_out = self.n_rows * (n_heads if self.per_head else 1)
        if self.gene_body and self.gene_maps is None:
            self.gene_maps = torch.empty((len(self.layers), n_out, max_k), dtype=torch.float32, device=q.device)
        if compact:
            assert q.shape[0] == self.n_rows and rows is None
        elif rows is not None:
            q_rows = rows[q_rows]
        if self.gene_body:
            ops.attn_probs(q, k, cu_rows, cu_k, 1, max_k, n_heads, head_dim, q_rows=q_rows, q_log2=True, per_head=self.per_head,
                           out=self.gene_maps[slot], family=family + "_maps", slopes=slopes, q_pos=None, k_rows=rows)
        if not self.gene_contributions:
            return
        assert cu_rows.numel() - 1 == self.n_rows           # one selected row per sequence: row s belongs to sequence s
        if self.gene_contrib is None:
            self.gene_contrib = torch.empty((len(self.layers), n_out, max_k), dtype=torch.float32, device=q.device)
            if not (self.per_head and self.gene_body):
                self._self_scratch = torch.empty((self.n_rows * n_heads, max_k), dtype=torch.float32, device=q.device)
        if self.per_head and self.gene_body:
            probs = self.gene_maps[slot]
        else:
            probs = self._self_scratch
            ops.attn_probs(q, k, cu_rows, cu_k, 1, max_k, n_heads, head_dim, q_rows=q_rows, q_log2=True, per_head=True,
                           out=probs, family=family + "_gene_contrib", slopes=slopes, q_pos=None, k_rows=rows)
        ops.attn_contrib_self(v, wo, probs, cu_k, max_k, n_heads, head_dim, out=self.gene_contrib[slot], per_head=self.per_head,
                              v_rows=rows, family=family + "_gene_contrib")


class _Layer:
    def __init__(self, cap: Capture, i: int, compact: bool):
        self.cap, self.i, self.compact = cap, i, compact

    def __enter__(self):
        self.prev = self.cap._running
        self.cap._running = (self.cap.layers.index(self.i), self.compact) if self.i in self.cap.layers else None
        return self

    def __exit__(self, *exc):
        self.cap._running = self.prev
        return False


class _NoLayer:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_LAYER = _NoLayer()


def select_layers(n_layers: int, layers=None) -> list:
    """The gene-layer indices a request names: None = all, negative indices count from the end; ValueError when an index is out
    of range, when none is given, or when two name the same layer (every slot of the result is one layer's map, written once).
    (One statement of the convention, for the model API and for the tests' oracle-side reference.)"""
    sel = list(range(n_layers)) if layers is None else [int(i) for i in layers]
    if not sel:
        raise ValueError("attention maps: `layers` names no gene layer (None means all)")
    for k, i in enumerate(sel):
        if not -n_layers <= i < n_layers:
            raise ValueError(f"gene layer {i} out of range (the model has {n_layers} gene layers)")
        sel[k] = i % n_layers
    if len(set(sel)) != len(sel):
        raise ValueError(f"attention maps: `layers` names a gene layer twice ({sel})")
    return sel


TOP_K_MAX, TOP_K_MAX_WIDTH = 64, 16384         # VF_TOPK_MAX_K / VF_TOPK_MAX_N of include/vf_hip_topk.h


def select_top_k(top_k=None) -> int | None:
    """The `top_k` a request names: None (the full maps) or an int in 1 .. 64; ValueError otherwise (a bool or a float too)."""
    if top_k is None:
        return None
    if isinstance(top_k, bool) or not hasattr(top_k, "__index__") or not 1 <= int(top_k) <= TOP_K_MAX:
        raise ValueError(f"attention maps: top_k must be None or an int in 1 .. {TOP_K_MAX}, got {top_k!r}")
    return int(top_k)


def active() -> Capture | None:
    """The capture open in this context, or None."""
    return _CAP.get()


def gene_layer(i: int, compact: bool = False):
    """with attn_maps.gene_layer(i): ...  -- tells the open capture (if any) which gene layer runs inside the block."""
    cap = _CAP.get()
    return _NO_LAYER if cap is None else cap.layer(i, compact)


def running() -> Capture | None:
    """The open capture when a gene layer it asked for is running and its forward has named the selected rows; else None."""
    cap = _CAP.get()
    return cap if cap is not None and cap._running is not None and cap._rows is not None else None


def running_self() -> Capture | None:
    """running(), when the capture also asked for the gene-body maps or the gene-body contributions and its forward has named
    the self-attention grouping."""
    cap = running()
    return cap if cap is not None and (cap.gene_body or cap.gene_contributions) and cap._self is not None else None


class capture:
    """with attn_maps.capture(layers, per_head, gene_body, contributions, gene_contributions) as cap: every forward inside
    records the requested gene layers' maps (gene_body: also those of the self attention over the gene body; contributions:
    also the value-weighted norms of the cross attention, cap.contrib; gene_contributions: those of the self attention,
    cap.gene_contrib, with or without gene_body)."""

    def __init__(self, layers, per_head: bool = False, gene_body: bool = False, contributions: bool = False,
                 gene_contributions: bool = False):
        self.cap = Capture(layers, per_head, gene_body, contributions, gene_contributions)

    def __enter__(self) -> Capture:
        self.token = _CAP.set(self.cap)
        return self.cap

    def __exit__(self, *exc):
        _CAP.reset(self.token)
        return False
