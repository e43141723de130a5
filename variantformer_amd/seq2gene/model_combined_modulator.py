"""Seq2GenePredictorCombinedModulator on the MI355X HIP kernels.

Same constructor keywords, sub-module names / state-dict keys and predict_step contract as the reference
(seq2gene/model_combined_modulator.py:36-135, 399-538, 857-907) so that
ModelManager(cfg).load_model() and VCFProcessor drive it unchanged.

What is different by design (all exact re-orderings of the same arithmetic):
  * The 24-layer CRE stream never sees the tissue id (add_context_to_cres false), so it is evaluated
    ONCE per gene instead of once per requested tissue (reference repeat: :622-649).
  * Gene-layer cross attention has no positional bias, so the T tissue copies of a gene form one query
    block against the gene's single K/V projection of the CRE stream.
  * CRE-layer cross attention reads K/V = Wkv(Embedding(9)[labels]); Wkv is applied to the 9-row table
    once per layer and rows are gathered per label.
  * All windows of all genes of a batch go through seq2reg together (the reference's <=1024-window chunks,
    :760-785, are independent of each other), and the head is evaluated for all rows in one pass.
"""
from __future__ import annotations

import collections
import logging
import threading
import types
import weakref
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, attn_maps, ops, runtime, weights
from ..utils.constants import REF_CREs
from ..utils.functions import precision2dtype
from .modules.layers import (AddContext, ContextFlashAttentionEncoderLayer, ContextFlashCrossAttentionEncoderLayer,
                             FlashAttentionEncoderLayer, MultiRegistry, StartToken, TissueExpressionHeads, _as_tensor, ln_fold_enabled,
                             packed_linear, pad_input, trunk16_enabled, unpad_input)

logger = logging.getLogger(__name__)
MAX_WINDOW_SIZE = 30000000
MAX_CHUNK_SIZE = 1024


@dataclass
class PreparedBatch:
    """Device-resident inputs of one batch plus the host-known structure (sizes and index maps).
    Built by Seq2GenePredictorCombinedModulator.prepare_batch from a collate_fn_batching dict."""
    n_genes: int
    tissues: list                      # per gene: list[int]
    n_cre: list                        # per gene N_i
    n_chunk: list                      # per gene C_i
    cre_ids: torch.Tensor              # int64 [sum N, L]
    cre_pad: torch.Tensor              # uint8 [sum N, L]
    cre_tokens: int                    # valid tokens over all CRE windows
    gene_ids: torch.Tensor             # int64 [sum C, L]
    gene_pad: torch.Tensor
    gene_tokens: int
    labels: torch.Tensor               # int64 [sum N]
    cu_cre: torch.Tensor               # int32 [n_genes+1]           CRE tokens per gene
    max_cre: int
    cu_gene_self: torch.Tensor         # int32 [sum T + 1]           one sequence per (gene, tissue), G_i tokens
    max_gene: int
    cu_gene_cross: torch.Tensor        # int32 [n_genes+1]           T_i * G_i query rows per gene
    max_gene_cross: int
    gene_stream_idx: torch.Tensor      # int64 [sum T_i*G_i]: >=0 row of gene_x, <0 registry row -(t+1)
    registry_rows: torch.Tensor        # int64 [sum T]: row of each registry token in the gene stream
    total_tissue_rows: int
    registry_rows_host: np.ndarray = None
    cu_cre_host: np.ndarray = None
    cu_registry: torch.Tensor = None          # int32 [sum T + 1] = arange: one registry query per (gene, tissue)
    cu_registry_cross: torch.Tensor = None    # int32 [n_genes + 1]: T_i registry rows per gene
    max_tissues: int = 1
    cre_unique_inverse: torch.Tensor = None   # int64 [sum N]: row of each window in the de-duplicated cre_ids
    gene_unique_inverse: torch.Tensor = None
    cre_ctx: torch.Tensor = None              # int64 [windows]: cCRE label of every (de-duplicated) CRE window, for a
                                              # use_context CRE tokenizer (seq2reg/model.py:222-245); None otherwise
    cre_max_len: int = 0                      # longest CRE window / gene chunk in valid tokens (0: padded length);
    gene_max_len: int = 0                     # sizes the attention grid of seq2reg
    ready: object = None                      # event of the side-stream upload (None: tensors are ready)
    windows_total: tuple = (0, 0)             # (CRE windows, gene chunks) of the batch ...
    windows_embedded: tuple = (0, 0)          # ... and how many of them seq2reg embeds after exact de-duplication
    tissues_used: torch.Tensor = None         # int64 [k]: distinct registry rows (tissue ids) the batch holds

    def wait(self, stream=None) -> "PreparedBatch":
        """Make `stream` (default: the current one) wait for the side-stream upload of prepare_batch.  forward_prepared does
        this itself; anything else that reads the tensors (scripts, tests) calls it first.  Readers of cre_ids / gene_ids
        also mind cre_unique_inverse / gene_unique_inverse: with window de-duplication the id tensors hold DISTINCT windows."""
        if self.ready is not None:
            (stream or torch.cuda.current_stream(self.cre_ids.device)).wait_event(self.ready)
        return self


class _HostStager:
    """Pinned host staging for prepare_batch: named buffers in two generations (batch i + 1 is staged while batch i's upload
    may still be in flight; a generation is reused only after its upload event has completed), and a side stream for the
    uploads.  Tensors allocated on the side stream are handed to the compute stream with record_stream."""

    def __init__(self, device):
        self.device = device
        self.cuda = device.type == "cuda"
        self.bufs, self.events, self.gen = {}, [None, None], 0
        self.stream = torch.cuda.Stream(device=device) if self.cuda else None

    def begin(self):
        self.gen ^= 1
        ev = self.events[self.gen]
        if ev is not None:
            ev.synchronize()

    def get(self, name, shape, dtype) -> torch.Tensor:
        n = 1
        for v in shape:
            n *= int(v)
        key = (name, self.gen)
        buf = self.bufs.get(key)
        if buf is None or buf.dtype != dtype or buf.numel() < n:
            buf = torch.empty(max(n, 1) + max(n, 1) // 4, dtype=dtype, pin_memory=self.cuda)
            self.bufs[key] = buf
        return buf[:n].view(*[int(v) for v in shape])

    def upload(self, host: dict, widen=()):
        """host: name -> staged tensor or numpy array.  Returns (name -> device tensor, event or None); `widen` names are
        int32 on the host and int64 on the device (the kernels' id type)."""
        out = {}
        if not self.cuda:
            for k, v in host.items():
                t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.clone()
                out[k] = t.long() if k in widen else t
            return out, None
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            for k, v in host.items():
                if isinstance(v, np.ndarray):                       # small structure arrays: staged here
                    b = self.get("np_" + k, v.shape, torch.from_numpy(v[:0]).dtype)
                    b.copy_(torch.from_numpy(np.ascontiguousarray(v)))
                    v = b
                t = v.to(self.device, non_blocking=True)
                if k in widen:
                    t = t.long()
                t.record_stream(main)
                out[k] = t
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.events[self.gen] = ev
        return out, ev


def _context_kv_table(ctx_embedding: nn.Embedding, layer) -> torch.Tensor:
    """bf16 [9, 2D] = Wkv_layer(context embedding table); constant per weights, cached on the layer."""
    tab, mha = ctx_embedding.weight, layer.crossMHA.MHA
    return weights.derived(layer, "_vf_ctx_kv", (tab, mha.Wkv.weight, mha.Wkv.bias),
                           lambda: mha.project_kv(ops.cast16(tab.detach().float().contiguous())))


LN_HEAL_STICKY_AFTER = 2      # alerting batches among a model's last 16 finished ones (a RATE, 2 of 16 = the point where a
                              # second forward per alerting batch costs as much as running unfolded) after which the fold stays
                              # off FOR THAT MODEL


class HealState:
    """Bookkeeping of the self-healing LayerNorm fold, ONE PER MODEL INSTANCE (round-5 advice: it was per process, so a
    checkpoint that kept alerting in one thread switched the fold off for every healthy model too).  Counters and the sticky
    switch are guarded by a lock: predict_finish may run in several threads."""

    def __init__(self):
        self.lock = threading.Lock()
        self.finished = 0          # batches whose outputs were handed back
        self.batches = 0           # ... of which recomputed with the separate LayerNorm
        self.logged = False
        self.recent = collections.deque(maxlen=16)
        self.off = False           # sticky: this model runs unfolded from now on (forward_prepared's runtime.forward_env)


_MODELS = weakref.WeakSet()       # models that own a HealState (ln_fold_state() without an argument sums over them)


def heal_state(model) -> HealState:
    st = model.__dict__.get("_vf_heal")
    if st is None:
        st = HealState()
        object.__setattr__(model, "_vf_heal", st)
        _MODELS.add(model)
    return st


def ln_fold_state(model=None) -> dict:
    """The self-healing LayerNorm fold's bookkeeping, for drivers and logs: whether the fold is on, how many batches were
    finished / recomputed, whether it was switched off -- for `model`, or summed over every live model of the process.
    `switched_off_by_alerts`: the model's own sticky switch (WARNING-logged when it happens); `switched_off_for_process`:
    layers.ln_fold_disable() was called (an explicit, process-wide choice)."""
    from .modules import layers as _layers
    from .. import runtime
    states = [heal_state(model)] if model is not None else [heal_state(m) for m in list(_MODELS)]
    off_alerts = any(st.off for st in states)
    return {"enabled": not _layers._LN_FOLD_DISABLED and runtime.read_env().ln_fold and not off_alerts,
            "switched_off_for_process": bool(_layers._LN_FOLD_DISABLED), "switched_off_by_alerts": bool(off_alerts),
            "models": len(states),
            "batches_finished": int(sum(st.finished for st in states)),
            "batches_recomputed": int(sum(st.batches for st in states))}


def _heal_if_ln_fold_alert(flag, recompute, state: HealState):
    """Called where a batch's outputs were copied back.  `flag`: the batch's OWN alert bits (ops.ln_fold_alert_take, enqueued
    right behind the batch's last kernel on its stream -- a device int, or already an int): whether some row of a
    LayerNorm-folded stream of THIS batch left the regime the fold serves: |mean| > ops.LN_FOLD_RATIO_LIMIT standard
    deviations (rounding the UNCENTRED row to 16 bits costs accuracy there) or an element a scaled fp16
    copy could not hold.  Then the batch is RECOMPUTED with the separate LayerNorm on fp32 rows (layers.ln_fold_forced_off,
    thread-local: bit for bit a VF_LN_FOLD=0 run) and `recompute()`'s result is returned; degraded numbers never leave the
    model, however deep the caller pipelines predict_launch / predict_finish.  The reference's plain nn.LayerNorm
    (seq2gene/modules/layers.py:75-77,99-163) has no such regime.  Returns None when nothing tripped.
    `state`: the model's HealState.  When LN_HEAL_STICKY_AFTER of its last 16 finished batches alerted, the fold is switched
    off for THAT MODEL (WARNING); other models of the process are not affected."""
    bits = 0 if flag is None else int(flag.item() if isinstance(flag, torch.Tensor) else flag)
    with state.lock:
        state.finished += 1
        state.recent.append(bool(bits))
        if not bits:
            return None
        state.batches += 1
        first, state.logged = not state.logged, True
    from .modules import layers as _layers
    log = logging.getLogger("variantformer_amd")
    if first:
        log.info("variantformer_amd: a residual-stream row left the folded-LayerNorm regime (%s); the batch was recomputed with "
                 "the separate LayerNorm pass (same results as VF_LN_FOLD=0)",
                 " and ".join(w for b, w in ((1, "|mean| > %g standard deviations" % ops.LN_FOLD_RATIO_LIMIT),
                                             (2, "an element beyond the fp16 copies' range")) if bits & b))
    with _layers.ln_fold_forced_off():
        out = recompute()
    with state.lock:
        trip = not state.off and sum(state.recent) >= LN_HEAL_STICKY_AFTER
        if trip:
            state.off = True
            n_alert, n_recent = sum(state.recent), len(state.recent)
    if trip:
        log.warning("variantformer_amd: %d of the last %d batches tripped the folded-LayerNorm alert; the fold is OFF for this "
                    "model from now on (every batch takes the separate LayerNorm pass; set VF_LN_FOLD=0 to start that "
                    "way; state: model.ln_fold_state())", n_alert, n_recent)
    return out


class PredictHandle:
    """What predict_launch returns and predict_finish consumes.  OPAQUE: drivers pass it on, nothing else (its fields changed
    between rounds and will again)."""
    __slots__ = ("tissues", "pred", "emb", "model", "pb", "alert", "done")

    def __init__(self, tissues, pred, emb, model, pb, alert, done):
        self.tissues, self.pred, self.emb, self.model, self.pb, self.alert, self.done = tissues, pred, emb, model, pb, alert, done


_SIDE_STREAMS: dict = {}
_OVERLAP_SERIALIZE_FOR_DIAG = False     # scripts/probes/overlap_diag.py only: the two-stream plumbing with the streams serialised


def _side_stream(device, main=None):
    """The side stream that belongs to `main` (default: the current stream of `device`): one per main stream, so that two
    models driven from two threads / streams neither queue behind each other nor share a LayerNorm-fold alert flag."""
    main = torch.cuda.current_stream(device) if main is None else main
    key = (device.type, device.index, main.cuda_stream)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS.setdefault(key, torch.cuda.Stream(device=device))     # (two threads racing here agree on one)
    return _SIDE_STREAMS[key]


def modulator_forward_packed(ctx_embedding, cre_layers, gene_layers, cre_x, gene_x, labels, cu_cre, max_cre,
                             cu_gene_self, max_gene, cu_gene_cross=None, max_gene_cross=None, cu_cre_for_gene=None,
                             final_rows=None, use_res=False, gene_unique=None):
    """Interleaved CRE / gene layer stack on packed streams (reference model_combined_modulator.py:244-285; the
    two-module variant seq2gene/model.py:375-412 + layers.py:620-742,797-921 evaluates the same sequence: gene layer
    i reads the CRE stream after CRE layer i-1, gene layer 0 the raw CRE embeddings).
    cre_x fp32 [sum N, D] (one CRE stream per K/V group), gene_x fp32 [tokens_g, D], labels int64 [sum N].
    cu_gene_self: self-attention sequences of the gene stream; cu_gene_cross / cu_cre_for_gene: matching
    query / key groups for the gene->CRE cross attention (default: same grouping as self-attention)."""
    cq = cu_gene_self if cu_gene_cross is None else cu_gene_cross
    mq = max_gene if max_gene_cross is None else max_gene_cross
    ck = cu_cre if cu_cre_for_gene is None else cu_cre_for_gene
    cre, gene = cre_x, gene_x
    n = len(gene_layers)
    # 16-bit trunk (layers.trunk16_enabled): a layer's result goes to the next layer of its stack as 16-bit copy + row
    # statistics only; the last layer of each stack (returned below) and a stream that `use_res` adds to keep fp32 rows
    t16 = trunk16_enabled() and ln_fold_enabled(cre_x.shape[1])
    if ln_fold_enabled(cre_x.shape[1]):
        # LayerNorm folded into the GEMMs: the streams travel as (fp32, bf16 copy, row statistics); one pass makes the
        # triple for the raw CRE embeddings (gene layer 0 projects K/V from the copy, CRE layer 0 consumes all three)
        cre = ops.ln_stream(cre_x)
    with ops.scope("gene_stream"):
        # gene_unique = (chunk rows, registry table, index): the stream entering gene layer 0 consists of copies of these
        # rows (one copy of a gene's chunk rows per tissue), so its LayerNorm1 -> Wqkv projection is computed once per
        # distinct row (exact; the other 24 gene layers see rows that differ by tissue)
        qkv0 = None
        if gene_unique is not None and hasattr(gene_layers[0], "self_qkv_of_unique_rows"):
            # gene_x None: the caller left the stream to be built here -- from 16-bit copies of the distinct rows when the
            # layer reads nothing else (no fp32 rows are ever written), else by the fp32 row gather below
            want_stream = gene_x is None and not use_res
            r = gene_layers[0].self_qkv_of_unique_rows(*gene_unique, with_stream=want_stream)
            if r is not None:
                qkv0, gene = r if want_stream else (r, gene)
        if gene is None:                                # registry row + chunk rows per (gene, tissue) (:357-366, layers.py:508-521)
            gene = ops.gather_rows_f32(gene_unique[0], gene_unique[1], gene_unique[2])
            gene_x = gene
        kw0 = {} if qkv0 is None else {"self_qkv": qkv0}
        with attn_maps.gene_layer(0):
            gene = gene_layers[0].forward_packed(gene, cu_gene_self, max_gene, context=cre, cu_ctx=ck, max_ctx=max_cre,
                                                 cu_cross_q=cq, max_cross_q=mq, keep_x=not t16 or use_res or n == 1, **kw0)
    if use_res:                                     # gene-stream input added back after every gene layer (:253-254)
        gene = ops.add_rows(_as_tensor(gene), gene_x)
    log2c = None
    if (ctx_embedding is not None and n > 1 and runtime.switches().counted_context_keys and ctx_embedding.num_embeddings <= 16
            and cre_layers[0].crossMHA.MHA.head_dim in (32, 48, 64)):
        # how often each label occurs among a gene's CREs (the same for all CRE layers): log2, -inf for an absent label
        C = ctx_embedding.num_embeddings
        lens = (cu_cre[1:] - cu_cre[:-1]).long()
        gid = torch.repeat_interleave(torch.arange(lens.numel(), device=labels.device), lens, output_size=labels.numel())
        cnt = torch.zeros(lens.numel() * C, dtype=torch.float32, device=labels.device)
        cnt.index_add_(0, gid * C + labels.long().clamp(0, C - 1), torch.ones(labels.numel(), dtype=torch.float32, device=labels.device))
        log2c = torch.log2(cnt).view(lens.numel(), C).contiguous()
    def cre_layer(i, cre_in):
        with ops.scope("cre_stream"):
            if ctx_embedding is None:
                kw_ctx = {"context_kv": None}
            elif log2c is not None:
                # the context rows are copies of the 9 label embeddings: softmax over the distinct rows with log(count) added
                kw_ctx = {"context_counted": (_context_kv_table(ctx_embedding, cre_layers[i]), log2c, ctx_embedding.weight)}
            else:
                kw_ctx = {"context_kv": ops.gather_rows_bf16(_context_kv_table(ctx_embedding, cre_layers[i]), labels)}
            return cre_layers[i].forward_packed(cre_in, cu_cre, max_cre, cu_ctx=cu_cre, max_ctx=max_cre,
                                                keep_x=not t16 or i == n - 2, **kw_ctx)

    def gene_layer(i, gene_in, cre_i):
        with ops.scope("gene_stream"):
            if final_rows is not None and i == n - 1:
                # last gene layer: only the registry rows are consumed downstream -> compact [R, D] result
                rows, cu_rows, cu_cross_rows, max_cross_rows = final_rows
                with attn_maps.gene_layer(i, compact=True):       # the query buffer already is the registry rows
                    return gene_layers[i].forward_packed_rows(gene_in, cu_gene_self, max_gene, rows, cu_rows, cre_i, ck, max_cre,
                                                              cu_cross_rows, max_cross_rows)
            with attn_maps.gene_layer(i):
                g = gene_layers[i].forward_packed(gene_in, cu_gene_self, max_gene, context=cre_i, cu_ctx=ck, max_ctx=max_cre,
                                                  cu_cross_q=cq, max_cross_q=mq, keep_x=not t16 or use_res or i == n - 1)
            if use_res:                                 # :284-285
                g = ops.add_rows(_as_tensor(g), gene_x)
            return g

    # runtime.Switches.overlap_cre_stream (default on): the CRE layers on a SIDE STREAM beside the gene layers -- CRE layer i + 1
    # depends on CRE layer i only, gene layer i + 1 on gene layer i and CRE layer i, so the small CRE-stream kernels (3-9 tiles
    # per CU) fill the tails of the gene stream's persistent GEMMs: -2 ... 4 ms per 32-gene step.  Every tensor that crosses
    # streams is event-ordered and recorded on its reader's stream.  Bit-identical to the single-stream order, at full depth and
    # run to run (tests/test_model_gpu.py), since the library has no packed-fp32 instruction (csrc/build.py).  A per-weights
    # cache a forward has to build is built on the main stream with the two streams joined (weights.build_streams).  Single
    # stream inside an ops.KernelTimer replay (per-kernel times must not depend on a neighbour).
    overlap = runtime.switches().overlap_cre_stream and n > 2 and ops.TIMER is None and _as_tensor(cre_x).is_cuda
    if not overlap:
        for i in range(n - 1):
            cre = cre_layer(i, cre)
            gene = gene_layer(i + 1, gene, cre)
        return _as_tensor(gene), _as_tensor(cre)
    dev = _as_tensor(cre_x).device
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev, main)

    def tensors(x):
        return [t for t in ((x.x, x.x16, x.stats, x.t16) if isinstance(x, ops.LnStream) else (x,)) if t is not None]

    def launch_cre(i, cre_in):
        with torch.cuda.stream(side):
            out = cre_layer(i, cre_in)
            ev = torch.cuda.Event()
            ev.record(side)
        for t in tensors(out):
            t.record_stream(main)
        if _OVERLAP_SERIALIZE_FOR_DIAG:                # scripts/probes/overlap_diag.py: the same plumbing, never two streams in flight
            main.wait_stream(side)
            side.wait_stream(main)
        return out, ev
    # (gene layer 0 above is already enqueued on the main stream: CRE layer 0 runs beside it)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        ops._alert_flag(dev).zero_()       # stale bits on the side stream's flag (an op-level call, an aborted forward) are nobody's
    with weights.build_streams(main, side):
        pending = launch_cre(0, cre)
        for i in range(n - 1):
            cre, ev = pending
            if i + 1 < n - 1:
                pending = launch_cre(i + 1, cre)
            main.wait_event(ev)
            gene = gene_layer(i + 1, gene, cre)
    with torch.cuda.stream(side):
        side_flag = ops._alert_flag(dev)
    main.wait_stream(side)
    ops._alert_flag(dev).bitwise_or_(side_flag)          # the side stream's LayerNorm-fold alerts belong to this batch too
    side_flag.zero_()
    side.wait_stream(main)
    return _as_tensor(gene), _as_tensor(cre)


class CombinedModulator(nn.Module):
    """24 CRE layers + 25 gene layers, interleaved, on packed streams
    (reference model_combined_modulator.py:36-328)."""

    def __init__(self, emb_dim, num_heads, num_layers, use_alibi, mlp_dout, use_context, num_ref_cres=None,
                 only_cross_attention=True, use_res=False, cross_alibi=False, flash_attn_3=False):
        super().__init__()
        self.emb_dim, self.num_heads, self.num_layers = emb_dim, num_heads, num_layers
        self.use_context, self.only_cross_attention = use_context, only_cross_attention
        self.use_res, self.cross_alibi = use_res, cross_alibi
        if use_context:
            assert num_ref_cres is not None, "num_ref_cres must be provided when use_context is True"
            self.second_level_context_embedding = nn.Embedding(num_ref_cres, emb_dim)
            # the CRE layers are built WITHOUT cross_alibi in the reference (:78-88); only the gene layers receive it
            mk_cre = lambda: ContextFlashAttentionEncoderLayer(  # noqa: E731
                d_model=emb_dim, nhead=num_heads, batch_first=True, use_alibi=use_alibi, mlp_dout=mlp_dout,
                flash_attn_3=flash_attn_3)
        else:                                   # context-free CRE layers (:89-103)
            self.second_level_context_embedding = None
            mk_cre = lambda: FlashAttentionEncoderLayer(  # noqa: E731
                d_model=emb_dim, nhead=num_heads, batch_first=True, use_alibi=use_alibi, mlp_dout=mlp_dout)
        gene_cls = ContextFlashCrossAttentionEncoderLayer if only_cross_attention else ContextFlashAttentionEncoderLayer
        mk = lambda: gene_cls(  # noqa: E731
            d_model=emb_dim, nhead=num_heads, batch_first=True, use_alibi=use_alibi, mlp_dout=mlp_dout,
            cross_alibi=cross_alibi, flash_attn_3=flash_attn_3)
        self.cre_layers = nn.ModuleList([mk_cre() for _ in range(num_layers - 1)])
        self.gene_layers = nn.ModuleList([mk() for _ in range(num_layers)])
        for stream, layers in (("cre", self.cre_layers), ("gene", self.gene_layers)):     # KernelTimer families
            for l in layers:
                if hasattr(l, "mixer"):
                    l.mixer.MHA.family = f"{stream}_self"
                if hasattr(l, "crossMHA"):
                    l.crossMHA.MHA.family = "cre_ctx_cross" if stream == "cre" else "gene_cre_cross"

    def forward_packed(self, cre_x, gene_x, labels, cu_cre, max_cre, cu_gene_self, max_gene, cu_gene_cross=None,
                       max_gene_cross=None, cu_cre_for_gene=None, final_rows=None, gene_unique=None):
        return modulator_forward_packed(self.second_level_context_embedding, self.cre_layers, self.gene_layers, cre_x,
                                        gene_x, labels, cu_cre, max_cre, cu_gene_self, max_gene, cu_gene_cross,
                                        max_gene_cross, cu_cre_for_gene, final_rows, use_res=self.use_res,
                                        gene_unique=gene_unique)

    def forward(self, cre_x, gene_x, context=None, cre_padding_mask=None, gene_padding_mask=None,
                context_padding_mask=None, precision=None, cre_token_position=None, gene_token_position=None):
        """Reference signature on padded, per-tissue-repeated tensors (:137-328).  No de-duplication is
        possible at this level (the caller already materialised the copies); same kernels otherwise."""
        B, Nc = cre_x.shape[:2]
        G = gene_x.shape[1]
        dev = cre_x.device
        if cre_padding_mask is None:
            cre_padding_mask = torch.zeros((B, Nc), dtype=torch.bool, device=dev)
        if gene_padding_mask is None:
            gene_padding_mask = torch.zeros((B, G), dtype=torch.bool, device=dev)
        cre_p, cre_idx, cu_c, max_c, _ = unpad_input(cre_x, ~cre_padding_mask)
        gene_p, gene_idx, cu_g, max_g, _ = unpad_input(gene_x, ~gene_padding_mask)
        labels = context.reshape(-1)[cre_idx].long().contiguous() if (self.use_context and context is not None) else None
        gene_out, cre_out = self.forward_packed(cre_p, gene_p, labels, cu_c, max_c, cu_g, max_g)
        gene_current = pad_input(gene_out, gene_idx, B, G)
        cre_current = pad_input(cre_out, cre_idx, B, Nc)
        ar = torch.arange(B, device=dev)
        if gene_token_position is not None:
            gene_tok = gene_current[ar, gene_token_position.long().reshape(-1), :]
        else:
            gene_tok = torch.zeros(B, gene_current.size(2), device=dev)
        if cre_token_position is not None:
            cre_tok = cre_current[ar, cre_token_position.long().reshape(-1), :]
        else:
            cre_tok = torch.zeros(B, cre_current.size(2), device=dev)
        return gene_current, gene_tok, cre_tok

    def prepare_input(self, g_exp, gene_pooling, start_tkn=None, tissue_vector=None, padding_mask_gene=None):
        """Reference :330-368 (multi_registry branch)."""
        res = g_exp.clone()
        if gene_pooling == "multi_registry" and start_tkn is not None:
            g_exp, res = start_tkn(g_exp, tissue_vector)
            if padding_mask_gene is not None:
                start = torch.zeros((padding_mask_gene.size(0), 1), dtype=padding_mask_gene.dtype,
                                    device=padding_mask_gene.device)
                padding_mask_gene = torch.cat((start, padding_mask_gene), dim=1)
        return g_exp, res, padding_mask_gene

    def pool_outputs(self, g_exp, gene_pooling, padding_mask_gene=None):
        """Reference :370-396; only the registry-token pooling of the shipped config."""
        if gene_pooling in ["start_token", "multi_registry"]:
            return g_exp[:, 0, :]
        raise NotImplementedError(f"gene pooling {gene_pooling!r} is not on the shipped path")


class Seq2GenePredictorCombinedModulator(nn.Module):
    def __init__(self, num_tissues: int, emb_dim: int, gene_emb_dim: int, num_heads: int, num_layers: int,
                 use_alibi: bool = True, mlp_dout: float = 0.1, weight_decay: float = 0.0, learning_rate: float = 1e-4,
                 lr_scale: float = 1, use_context: bool = False, token_dim: int = 128, cre_tokenizer=None,
                 gene_tokenizer=None, cre_tokenizer_train_mode="val", cre_tokenizer_val_mode="val",
                 gene_tokenizer_train_mode="val", gene_tokenizer_val_mode="val", tissues: list = None,
                 optimizer="adam", gene_pooling="mean", flash_attn_3=False, **kwargs):
        super().__init__()
        hp = dict(num_tissues=num_tissues, emb_dim=emb_dim, gene_emb_dim=gene_emb_dim, num_heads=num_heads,
                  num_layers=num_layers, use_alibi=use_alibi, mlp_dout=mlp_dout, use_context=use_context,
                  token_dim=token_dim, gene_pooling=gene_pooling, flash_attn_3=flash_attn_3)
        hp.update(kwargs)
        self.hparams = types.SimpleNamespace(**hp)
        self.trainer = None
        self.vep = False
        self.precision = None
        assert gene_pooling in ["mean", "max", "start_token", "multi_registry"], \
            "gene_pooling must be one of mean, max, start_token, or multi_registry"
        if gene_pooling == "mean":
            raise NotImplementedError("gene_pooling='mean' does not reduce over tokens in the reference "
                                      "(model_combined_modulator.py:375-378) and cannot feed the heads")
        self.gene_pooling = gene_pooling
        self.start_tkn = (MultiRegistry(num_tissues, emb_dim) if gene_pooling == "multi_registry" else
                          StartToken(emb_dim) if gene_pooling == "start_token" else None)
        self.train_gene_tokenizer = kwargs.get("train_gene_tokenizer", False)
        self.cre_tokenizer = cre_tokenizer
        self.gene_tokenizer = gene_tokenizer
        self.add_context_to_cres = kwargs.get("add_context_to_cres", False)
        self.add_context = AddContext(num_tissues, emb_dim) if self.add_context_to_cres else None
        self.emb_dim = emb_dim
        self.use_context = use_context
        self.tissues = tissues
        self.use_res = kwargs.get("use_res", False)
        self.loss_fn = kwargs.get("loss_fn", "poisson")
        self.use_bigger_head = kwargs.get("use_bigger_head", False)
        self.multi_head = kwargs.get("multi_head", True)
        self.only_cross_attention = kwargs.get("only_cross_attention", True)
        self.cross_alibi = kwargs.get("cross_alibi", False) if use_alibi else False
        self.gene_map = nn.Linear(gene_emb_dim, emb_dim)
        if token_dim != emb_dim:
            self.cre_map = nn.Linear(token_dim, emb_dim)
        # Any option the shipped configuration leaves off takes the literal evaluation order of the reference (one CRE
        # stream and one gene stream per (gene, tissue), no sharing); same kernels, `_forward_general`.
        self._general = (self.only_cross_attention or self.use_res or self.cross_alibi or self.add_context_to_cres
                         or gene_pooling != "multi_registry")
        self._build_modulator(emb_dim, num_heads, num_layers, use_alibi, mlp_dout, use_context, flash_attn_3)
        self.tissue_heads = TissueExpressionHeads(emb_dim, num_tissues, use_bigger_head=self.use_bigger_head,
                                                  multi_head=self.multi_head, mlp_dout=mlp_dout, loss_fn=self.loss_fn,
                                                  head_type=kwargs.get("head_type", "mlp"))
        for p in self.parameters():            # inference-only build
            p.requires_grad_(False)

    # ---------------------------------------------------------------------------------------------
    def _build_modulator(self, emb_dim, num_heads, num_layers, use_alibi, mlp_dout, use_context, flash_attn_3):
        self.combined_modulator = CombinedModulator(
            emb_dim=emb_dim, num_heads=num_heads, num_layers=num_layers, use_alibi=use_alibi, mlp_dout=mlp_dout,
            use_context=use_context, num_ref_cres=len(REF_CREs) if use_context else None,
            only_cross_attention=self.only_cross_attention, use_res=self.use_res, cross_alibi=self.cross_alibi,
            flash_attn_3=flash_attn_3)

    def _modulator_forward_packed(self, *a, **k):
        return self.combined_modulator.forward_packed(*a, **k)

    @property
    def device(self):
        return self.gene_map.weight.device

    def operand_dtype(self):
        """16-bit operand type of the GEMM / attention kernels for the trainer's precision string (reference
        utils/functions.py:12-32 + model_combined_modulator.py:736-744 + layers.py:102-125):
          "bf16-mixed" (shipped, configs/vf_model.yaml:37) -> bf16 operands, fp32 accumulation;
          "16-mixed" / "16"                                -> fp16 operands, fp32 accumulation (autocast fp16);
          "32" / "32-true"                                 -> the reference keeps fp32 outside the MHA modules and runs
                                                              those in fp16; here every GEMM takes fp16 operands (10-bit
                                                              mantissa, the closest MFMA type) with fp32 accumulation.
        No trainer attached -> the shipped bf16.  `self.precision` (a string) overrides the trainer."""
        p = self.precision if isinstance(self.precision, str) else getattr(self.trainer, "precision", None)
        if p is None:
            return torch.bfloat16
        return torch.bfloat16 if precision2dtype(str(p)) == torch.bfloat16 else torch.float16

    def _precision_branch(self):
        """Reference :736-744: bf16/fp16-mixed -> None (autocast path), anything else -> fp32 (which the
        reference then runs through an fp16 flash-attn round trip).  The value is what transform_with_batching
        returns; the operand type the kernels use comes from operand_dtype()."""
        try:
            p = precision2dtype(self.trainer.precision)
        except Exception:
            p = torch.float32
        return None if p in (torch.float16, torch.bfloat16) else torch.float32

    @staticmethod
    def _unique_windows(ids: np.ndarray, pad: np.ndarray, extra: np.ndarray | None = None, _force_collisions: bool = False):
        """Exact de-duplication of windows: rows of (ids int32 [W, L], pad uint8 [W, L][, extra int [W]]) that are identical in
        every element are embedded once (seq2reg sees windows independently; `extra` = the window's context label when the
        tokenizer reads it).  Returns (keep, inverse): sorted first-occurrence rows, and for every window the index of its
        representative in `keep`; or None when no two rows are equal.
        A 64-bit multiply-add hash of each row groups the candidates (np.unique over W words instead of over a [W, 2L]
        matrix: 39 k windows of a 32-gene batch in ~5 ms instead of ~1 s); every group is then VERIFIED element by element
        against its representative, and a hash collision falls back to the row-wise np.unique -- the result never depends on
        the hash."""
        W, L = ids.shape
        if W < 2:
            return None
        key = ids.astype(np.int32, copy=False) ^ (pad.astype(np.int32) << 30)       # ids < 2^30 (checked by the caller)
        if L % 2:
            key = np.concatenate([key, np.zeros((W, 1), np.int32)], axis=1)
        k64 = np.ascontiguousarray(key).view(np.uint64)                             # [W, ceil(L / 2)]
        mult = (np.arange(1, k64.shape[1] + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
        if _force_collisions:                                                       # tests: every row gets the same hash
            mult = np.zeros_like(mult)
        with np.errstate(over="ignore"):
            h = (k64 * mult[None, :]).sum(axis=1, dtype=np.uint64)
            if extra is not None and not _force_collisions:
                h = h * np.uint64(0xD6E8FEB86659FD93) + extra.astype(np.uint64).reshape(-1)
        _, first, inverse = np.unique(h, return_index=True, return_inverse=True)
        inverse = inverse.reshape(-1)
        if len(first) == W:
            return None                                                             # all rows distinct: nothing to share
        rep = first[inverse]
        dup = np.nonzero(rep != np.arange(W))[0]                                    # rows that claim a representative
        same = (key[dup] == key[rep[dup]]).all(axis=1)
        if extra is not None:
            same &= extra.reshape(-1)[dup] == extra.reshape(-1)[rep[dup]]
        if not same.all():                                                          # a 64-bit collision: exact grouping
            cols = [key] + ([extra.astype(np.int32).reshape(-1, 1)] if extra is not None else [])
            _, first, inverse = np.unique(np.concatenate(cols, axis=1), axis=0, return_index=True, return_inverse=True)
            inverse = inverse.reshape(-1)
        order = np.argsort(first)                       # keep first-occurrence order
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        return np.sort(first), rank[inverse].astype(np.int64)

    def _stager(self):
        st = getattr(self, "_vf_stager", None)
        if st is None or st.device != self.device:
            st = _HostStager(self.device)
            object.__setattr__(self, "_vf_stager", st)
        return st

    def prepare_batch(self, batch: dict, dedupe_windows: bool | None = None) -> PreparedBatch:
        """collate_fn_batching dict (datasets/vcfdataset.py:18-63) -> device tensors + structure.
        Host work per batch: the per-gene id / mask tensors are copied ONCE, narrowed (int64 -> int32, bool -> uint8), into
        pinned staging buffers that are reused from batch to batch, and uploaded on a side stream (the copy engines run
        while the previous batch computes; round 3 concatenated int64 tensors in pageable memory and uploaded them on the
        compute stream: 155-233 ms per 32-gene batch).  forward_prepared waits for the upload's event.
        dedupe_windows: embed identical CRE windows / gene chunks once -- exact (see _unique_windows).  None (default): on
        whenever it removes windows (neighbouring genes of a whole-genome scan share cCRE windows byte for byte, reference
        datasets/vcfdataset.py:219-283; VEP ref / het / hom batches share all but the windows that carry the variant,
        datasets/vepdataset.py:347-477); False: off; True: same as None."""
        dev = self.device
        x, m = batch["cre_sequences"], batch["cre_attention_masks"]
        gx, gm = batch["gene_embeddings"], batch["gene_attention_masks"]
        n_genes = len(x)
        tissues = [[int(t) for t in tv] for tv in batch["tissue_context"]]
        n_cre = [int(v.shape[0]) for v in x]
        n_chunk = [int(v.shape[0]) for v in gx]
        for v in list(x) + list(gx):
            assert v.shape[1] == 1, "one strand per window (strand is picked in the dataloader)"
        st = self._stager()
        st.begin()
        id_flags = {}                                # per id array: bit 0 = a negative id, bit 1 = an id >= 2^30

        def gather(name, parts, dtype):
            """per-gene [n_i, 1, L] tensors -> one staged [sum n_i, L] array of `dtype`: one narrowing copy per gene, by numpy
            (single-threaded: torch's copy_ forks an OpenMP team per call, which collides with the loader workers when a rank
            has few host cores -- 170 ms instead of 25 per 32-gene batch on 2-4 cores, profiles/r04_c_host_capacity.log)"""
            L = int(parts[0].shape[2]) if len(parts) else 0
            buf = st.get(name, (sum(int(v.shape[0]) for v in parts), L), dtype)
            dst = buf.numpy()
            off = 0
            for v in parts:
                n = int(v.shape[0])
                if v.device.type != "cpu":
                    # a device-resident input: ONE copy into a pinned staging slice (a .cpu() per gene allocated pageable
                    # memory and synchronised each time; round-5 advice), narrowed from there like a host input
                    raw = st.get(name + "_raw", (n, 1, L), v.dtype)
                    raw.copy_(v)
                    v = raw
                src = v.numpy()[:, 0, :]
                if dtype == torch.uint8:                          # masks: exactly 0 / 1 whatever the caller's dtype holds
                    if src.dtype == np.bool_:
                        np.copyto(dst[off:off + n], src, casting="unsafe")
                    else:
                        np.not_equal(src, 0, out=dst[off:off + n].view(np.bool_))
                elif n:                                           # ids: the kernels clamp to [0, vocab); narrowing must not wrap first
                    if src.dtype == np.int64 and src.strides[1] == 8 and src.strides[0] % 8 == 0:
                        # one native pass: clamp to [-1, INT32_MAX] (the same token as the int64 path's clamp), narrow, and report
                        # what the ids looked like (bit 0: negative, bit 1: >= 2^30)
                        f = _lib.load().vf_narrow_ids(src.ctypes.data, src.strides[0] // 8, dst[off:off + n].ctypes.data, n, L)
                        if f < 0:
                            raise _lib.VFError("vf_narrow_ids: bad arguments")
                        id_flags[name] = id_flags.get(name, 0) | f
                    else:
                        lo, hi = int(src.min()), int(src.max())
                        id_flags[name] = id_flags.get(name, 0) | (1 if lo < 0 else 0) | (2 if hi >= 2 ** 30 else 0)
                        if src.dtype.itemsize > 4 and (lo < -1 or hi > 2 ** 31 - 1):
                            src = np.clip(src, -1, 2 ** 31 - 1)
                        np.copyto(dst[off:off + n], src, casting="unsafe")
                off += n
            return buf
        cre_ids, cre_pad = gather("cre_ids", x, torch.int32), gather("cre_pad", m, torch.uint8)
        gene_ids, gene_pad = gather("gene_ids", gx, torch.int32), gather("gene_pad", gm, torch.uint8)
        n_lab = sum(int(v.numel()) for v in batch["ref_cre_labels"])
        labels = st.get("labels", (n_lab,), torch.int64)
        off = 0
        for v in batch["ref_cre_labels"]:
            labels[off:off + v.numel()].copy_(torch.as_tensor(v).reshape(-1))
            off += v.numel()
        use_ctx = getattr(self.cre_tokenizer, "use_context", False)
        cre_keep = gene_keep = cre_inv = gene_inv = None
        cre_ctx = labels if use_ctx else None
        if dedupe_windows is not False:
            cre_np, gene_np = cre_ids.numpy(), gene_ids.numpy()
            # the 64-bit row key packs (id | pad << 30): ids must lie in [0, 2^30) (seen while narrowing)
            if id_flags.get("cre_ids", 0) or id_flags.get("gene_ids", 0):
                if not getattr(self, "_vf_dedupe_gate_logged", False):       # once per model: the batch still runs, undeduplicated
                    object.__setattr__(self, "_vf_dedupe_gate_logged", True)
                    logger.info("variantformer_amd: window de-duplication skipped for a batch that holds token ids outside "
                                "[0, 2^30) (a negative or very large id anywhere in the batch: the 64-bit row key packs id | pad << 30); "
                                "results are unaffected, seq2reg embeds every window (PreparedBatch.windows_embedded == windows_total)")
            else:
                r = self._unique_windows(cre_np, cre_pad.numpy(), labels.numpy() if use_ctx else None)
                if r is not None:
                    cre_keep, cre_inv = r
                r = self._unique_windows(gene_np, gene_pad.numpy())
                if r is not None:
                    gene_keep, gene_inv = r

        def select(buf, keep, name):
            if keep is None:
                return buf
            out = st.get(name, (len(keep),) + tuple(buf.shape[1:]), buf.dtype)
            torch.index_select(buf, 0, torch.from_numpy(keep), out=out)
            return out
        cre_ids, cre_pad = select(cre_ids, cre_keep, "cre_ids_u"), select(cre_pad, cre_keep, "cre_pad_u")
        gene_ids, gene_pad = select(gene_ids, gene_keep, "gene_ids_u"), select(gene_pad, gene_keep, "gene_pad_u")
        if cre_ctx is not None and cre_keep is not None:
            cre_ctx = select(cre_ctx, cre_keep, "cre_ctx_u")       # label of the first occurrence of every kept window

        def valid_counts(pad):
            if pad.numel() == 0:
                return 0, 0
            lens = pad.shape[1] - pad.numpy().sum(axis=1, dtype=np.int64)
            return int(lens.sum()), int(lens.max())
        cre_tokens, cre_max_len = valid_counts(cre_pad)
        gene_tokens, gene_max_len = valid_counts(gene_pad)
        # structure
        cu_cre = np.concatenate([[0], np.cumsum(n_cre)]).astype(np.int32)
        self_lens, cross_lens, idx, reg_rows = [], [], [], []
        gx_off, row = 0, 0
        for i in range(n_genes):
            G = n_chunk[i] + 1
            chunk_rows = np.arange(gx_off, gx_off + n_chunk[i], dtype=np.int64)
            for t in tissues[i]:
                self_lens.append(G)
                reg_rows.append(row)
                idx.append(np.concatenate([[-(t + 1)], chunk_rows]))
                row += G
            cross_lens.append(G * len(tissues[i]))
            gx_off += n_chunk[i]
        cu_self = np.concatenate([[0], np.cumsum(self_lens)]).astype(np.int32)
        cu_cross = np.concatenate([[0], np.cumsum(cross_lens)]).astype(np.int32)
        host = dict(
            cre_ids=cre_ids, cre_pad=cre_pad, gene_ids=gene_ids, gene_pad=gene_pad, labels=labels,
            cu_cre=cu_cre, cu_gene_self=cu_self, cu_gene_cross=cu_cross, gene_stream_idx=np.concatenate(idx),
            registry_rows=np.array(reg_rows, dtype=np.int64), cu_registry=np.arange(len(reg_rows) + 1, dtype=np.int32),
            cu_registry_cross=np.concatenate([[0], np.cumsum([len(t) for t in tissues])]).astype(np.int32))
        host["tissues_used"] = np.unique(np.array([t for ts in tissues for t in ts], dtype=np.int64))
        if cre_ctx is not None:
            host["cre_ctx"] = cre_ctx
        if cre_inv is not None:
            host["cre_unique_inverse"] = cre_inv
        if gene_inv is not None:
            host["gene_unique_inverse"] = gene_inv
        d, ready = st.upload(host, widen=("cre_ids", "gene_ids"))
        return PreparedBatch(
            n_genes=n_genes, tissues=tissues, n_cre=n_cre, n_chunk=n_chunk,
            cre_ids=d["cre_ids"], cre_pad=d["cre_pad"], cre_tokens=cre_tokens,
            gene_ids=d["gene_ids"], gene_pad=d["gene_pad"], gene_tokens=gene_tokens,
            labels=d["labels"], cu_cre=d["cu_cre"], max_cre=max(n_cre), cu_gene_self=d["cu_gene_self"],
            max_gene=max(self_lens), cu_gene_cross=d["cu_gene_cross"], max_gene_cross=max(cross_lens),
            gene_stream_idx=d["gene_stream_idx"], registry_rows=d["registry_rows"],
            cre_max_len=cre_max_len, gene_max_len=gene_max_len, cre_ctx=d.get("cre_ctx"),
            total_tissue_rows=len(reg_rows), registry_rows_host=np.array(reg_rows, dtype=np.int64), cu_cre_host=cu_cre,
            cu_registry=d["cu_registry"], cu_registry_cross=d["cu_registry_cross"],
            max_tissues=max(len(t) for t in tissues),
            cre_unique_inverse=d.get("cre_unique_inverse"), gene_unique_inverse=d.get("gene_unique_inverse"),
            ready=ready, tissues_used=d["tissues_used"], windows_total=(sum(n_cre), sum(n_chunk)),
            windows_embedded=(int(cre_ids.shape[0]), int(gene_ids.shape[0])))

    def forward_prepared(self, pb: PreparedBatch, return_cre: bool = False):
        """The hot path: everything below runs as HIP kernels on the current stream.
        Returns (pred fp32 [sum T, 1], emb fp32 [sum T, D])."""
        pb.wait()                                        # the side-stream upload of prepare_batch
        # one read of VF_LN_FOLD / VF_TRUNK16 for the whole forward, and this model's own sticky switch of the self-healing fold
        with ops.compute_dtype(self.operand_dtype()), runtime.forward_env(fold_off=heal_state(self).off):
            return self._forward_prepared(pb, return_cre)

    def ln_fold_state(self) -> dict:
        """ln_fold_state(self): this model's share of the self-healing LayerNorm fold's bookkeeping."""
        return ln_fold_state(self)

    def _forward_prepared(self, pb: PreparedBatch, return_cre: bool = False):
        # seq2reg over every CRE window / gene chunk of the batch (HOT LOOP A)
        cre_tok = self.cre_tokenizer.embed_packed(pb.cre_ids, pb.cre_pad, pb.cre_tokens, max_len=pb.cre_max_len,
                                                  context=pb.cre_ctx)                                          # 16-bit [sum N, d]
        gene_tokenizer = self.gene_tokenizer if self.gene_tokenizer is not None else self.cre_tokenizer
        gene_tok = gene_tokenizer.embed_packed(pb.gene_ids, pb.gene_pad, pb.gene_tokens, max_len=pb.gene_max_len)        # bf16 [sum C, d]
        if pb.cre_unique_inverse is not None:            # de-duplicated windows -> one row per original window
            cre_tok = ops.gather_rows_bf16(cre_tok, pb.cre_unique_inverse)
        if pb.gene_unique_inverse is not None:
            gene_tok = ops.gather_rows_bf16(gene_tok, pb.gene_unique_inverse)
        # maps (:610-612)
        if hasattr(self, "cre_map"):
            w, b = packed_linear(self.cre_map)
            cre_x = ops.gemm(cre_tok, w, b, ops.EPI_F32)
        else:
            cre_x = cre_tok.float()
        w, b = packed_linear(self.gene_map)
        gene_x = ops.gemm(gene_tok, w, b, ops.EPI_F32)
        cap = attn_maps.active()
        if cap is not None:
            # the maps' rows are the registry-token rows -- the only rows the expression head reads; pb.registry_rows already
            # indexes the buffer the gene layers' cross attention projects its queries from (the gene stream itself)
            self._attention_maps_supported(vep_ok=True)
            # the same rows are position 0 of the gene stream's self-attention sequences (registry token + chunks): one row per
            # sequence, the grouping the last layer's registry-rows form already uses
            cap.begin(pb.registry_rows, pb.cu_registry_cross, pb.max_tissues, pb.cu_cre, pb.max_cre,
                      gene_self=(pb.cu_registry, pb.cu_gene_self, pb.max_gene),
                      shape=([len(t) for t in pb.tissues], list(pb.n_cre), list(pb.n_chunk)))
        if self._general:
            return self._forward_general(pb, cre_x, gene_x, return_cre)
        # registry token per (gene, tissue) + that gene's chunk rows (:357-366, layers.py:508-521)
        # what the gene stream's rows are copies of (+ the registry rows in use: only they may raise the LayerNorm-fold alert);
        # modulator_forward_packed builds the stream from it (gene_stream = None)
        gene_stream = None
        uniq = (gene_x, self.start_tkn.registry_tokens.weight, pb.gene_stream_idx, pb.tissues_used)
        if return_cre:       # VEP needs every gene token of the last layer (token-position gathers)
            gene_out, cre_out = self._modulator_forward_packed(
                cre_x, gene_stream, pb.labels, pb.cu_cre, pb.max_cre, pb.cu_gene_self, pb.max_gene,
                cu_gene_cross=pb.cu_gene_cross, max_gene_cross=pb.max_gene_cross, gene_unique=uniq)
            emb = ops.gather_rows_f32(gene_out, None, pb.registry_rows)                         # pool_outputs (:391-392)
        else:                # only row 0 (registry token) of the last gene layer is consumed: compute just those rows
            emb, cre_out = self._modulator_forward_packed(
                cre_x, gene_stream, pb.labels, pb.cu_cre, pb.max_cre, pb.cu_gene_self, pb.max_gene,
                cu_gene_cross=pb.cu_gene_cross, max_gene_cross=pb.max_gene_cross,
                final_rows=(pb.registry_rows, pb.cu_registry, pb.cu_registry_cross, pb.max_tissues), gene_unique=uniq)
            gene_out = None
        pred = self.tissue_heads(emb, [t for ts in pb.tissues for t in ts])
        if return_cre:
            # row of gene chunk 0 / of CRE 0 of every (gene, tissue) output row inside gene_out / cre_out (the shared CRE
            # stream holds one copy per gene; +1: the registry token in front of the chunks, reference :665-666)
            gene_base = pb.registry_rows_host + 1
            cre_base = np.repeat(np.asarray(pb.cu_cre_host[:-1], dtype=np.int64), [len(t) for t in pb.tissues])
            return pred, emb, gene_out, cre_out, gene_base, cre_base
        return pred, emb

    def _forward_general(self, pb: PreparedBatch, cre_x: torch.Tensor, gene_x: torch.Tensor, return_cre: bool = False):
        """Literal evaluation order of the reference for the options the shipped configuration leaves off
        (reference :614-700): every (gene, tissue) pair owns a copy of the gene's CRE stream (plus the tissue embedding
        when add_context_to_cres) and a gene sequence (start / registry token in front, or none for max pooling); cross
        attention pairs sequence b of the gene stream with sequence b of the CRE stream (ALiBi when cross_alibi)."""
        dev = cre_x.device
        prefix = 0 if self.gene_pooling == "max" else 1
        cre_idx, cre_tissue, gene_idx, cre_lens, gene_lens = [], [], [], [], []
        c_off = 0
        for i in range(pb.n_genes):
            n, c = pb.n_cre[i], pb.n_chunk[i]
            n_off = int(pb.cu_cre_host[i])
            for t in pb.tissues[i]:
                cre_idx.append(np.arange(n_off, n_off + n, dtype=np.int64))
                cre_tissue.append(np.full(n, t, dtype=np.int64))
                head = [-(t + 1)] if self.gene_pooling == "multi_registry" else [-1] if prefix else []
                gene_idx.append(np.concatenate([np.asarray(head, dtype=np.int64), np.arange(c_off, c_off + c, dtype=np.int64)]))
                cre_lens.append(n)
                gene_lens.append(c + prefix)
            c_off += c
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        cre_idx = to(np.concatenate(cre_idx))
        cu_cre = to(np.concatenate([[0], np.cumsum(cre_lens)]).astype(np.int32))
        cu_gene = to(np.concatenate([[0], np.cumsum(gene_lens)]).astype(np.int32))
        if self.add_context is not None:                  # AddContext (layers.py:558-573)
            cre_rep = ops.add_rows(cre_x, self.add_context.registry_tokens.weight.float().contiguous(), cre_idx,
                                   to(np.concatenate(cre_tissue)))
        else:
            cre_rep = ops.gather_rows_f32(cre_x, None, cre_idx)
        labels_rep = pb.labels[cre_idx].contiguous()
        if self.gene_pooling == "multi_registry":
            table = self.start_tkn.registry_tokens.weight
        elif self.gene_pooling == "start_token":
            table = self.start_tkn.start_token.reshape(1, -1)
        else:
            table = None
        gene_stream = ops.gather_rows_f32(gene_x, None if table is None else table.float().contiguous(),
                                          to(np.concatenate(gene_idx)))
        gene_out, cre_out = self._modulator_forward_packed(cre_rep, gene_stream, labels_rep, cu_cre, max(cre_lens), cu_gene,
                                                           max(gene_lens))
        if self.gene_pooling == "max":                    # pool_outputs (:380-389)
            emb = ops.segment_max(gene_out, cu_gene)
        else:                                             # start / registry token (:391-392)
            emb = ops.gather_rows_f32(gene_out, None, cu_gene[:-1].long().contiguous())
        pred = self.tissue_heads(emb, [t for ts in pb.tissues for t in ts])
        if return_cre:       # every (gene, tissue) row owns a gene sequence (start token in front iff there is one, :665-666)
            gene_base = np.concatenate([[0], np.cumsum(gene_lens)])[:-1].astype(np.int64) + prefix
            cre_base = np.concatenate([[0], np.cumsum(cre_lens)])[:-1].astype(np.int64)
            return pred, emb, gene_out, cre_out, gene_base, cre_base
        return pred, emb

    def forward(self, inp, attention_mask, tissue_vector, cre_context, strand, gene_embedding, gene_att_mask,
                return_embedding=False, get_all=False, **kwargs):
        """Reference signature (:540-720).  Token-position outputs (VEP) come from variant_prediction."""
        batch = {"cre_sequences": inp, "cre_attention_masks": attention_mask, "tissue_context": tissue_vector,
                 "ref_cre_labels": cre_context, "strand_val": strand, "gene_embeddings": gene_embedding,
                 "gene_attention_masks": gene_att_mask}
        pb = self.prepare_batch(batch, dedupe_windows=kwargs.get("dedupe_windows"))
        donors = list(range(pb.n_genes))
        cre_pos, gene_pos = kwargs.get("cre_token_position"), kwargs.get("gene_token_position")
        if kwargs.get("only_embedding", False):
            return {"embedding": self.forward_prepared(pb)[1], "donors": donors}
        if not return_embedding:
            return self.forward_prepared(pb)[0], donors
        pred, emb, gene_out, cre_out, gene_base, cre_base = self.forward_prepared(pb, return_cre=True)
        gene_tok_emb = torch.zeros(pb.total_tissue_rows, self.emb_dim, device=pred.device)
        cre_tok_emb = torch.zeros(pb.total_tissue_rows, self.emb_dim, device=pred.device)
        if gene_pos is not None or cre_pos is not None:
            g_rows, c_rows, r = [], [], 0
            for i in range(pb.n_genes):
                for _ in pb.tissues[i]:
                    if gene_pos is not None:
                        g_rows.append(int(gene_base[r]) + int(torch.as_tensor(gene_pos[i]).reshape(-1)[0]))
                    if cre_pos is not None:
                        c_rows.append(int(cre_base[r]) + int(torch.as_tensor(cre_pos[i]).reshape(-1)[0]))
                    r += 1
            if g_rows:
                gene_tok_emb = ops.gather_rows_f32(gene_out, None, torch.tensor(g_rows, device=pred.device))
            if c_rows:
                cre_tok_emb = ops.gather_rows_f32(cre_out, None, torch.tensor(c_rows, device=pred.device))
        return pred, donors, emb, gene_tok_emb, cre_tok_emb

    def transform_with_batching(self, x, attention_mask, tissue_context, ref_labels_tensor, strand, embedder,
                                detach_embedding=True):
        """Reference :722-829: per-gene seq2reg embeddings stacked and padded to the longest gene.
        Returns (X [B,maxN,d] fp32, mask [B,maxN] bool True=pad, ref_labels [B,maxN] int64, precision, donors)."""
        precision = self._precision_branch()
        dev = self.device
        n = [int(v.shape[0]) for v in x]
        ids = torch.cat([v[:, 0, :] for v in x]).long().contiguous().to(dev)
        pad = torch.cat([v[:, 0, :] for v in attention_mask]).bool().contiguous().to(dev)
        ctx = None
        if getattr(embedder, "use_context", False):       # reference :778-785 hands the labels to the embedder
            ctx = torch.cat([torch.as_tensor(v).reshape(-1) for v in ref_labels_tensor]).to(dev)
        emb = embedder.embed_packed(ids, pad, int((~pad).sum().item()), torch.float32, context=ctx)
        maxn = max(n)
        X = torch.zeros((len(n), maxn, emb.shape[1]), dtype=torch.float32, device=dev)
        mask = torch.ones((len(n), maxn), dtype=torch.bool, device=dev)
        labels = torch.zeros((len(n), maxn), dtype=torch.long, device=dev)
        off = 0
        for i, ni in enumerate(n):
            X[i, :ni] = emb[off:off + ni]
            mask[i, :ni] = False
            labels[i, :ni] = torch.as_tensor(ref_labels_tensor[i]).to(dev).long()[:ni]
            off += ni
        return X, mask, labels, precision, list(range(len(n)))

    def predict_step(self, batch, batch_idx, dataloader_idx=None):
        """Reference :857-907: dict of per-gene fp32 numpy arrays."""
        self.eval()
        if self.vep:
            return self.variant_prediction(batch)
        with torch.no_grad():
            return self.predict_finish(self.predict_launch(self.prepare_batch(batch)), batch_idx, dataloader_idx)

    def _attention_maps_supported(self, vep_ok: bool = False) -> None:
        """Raises NotImplementedError naming the option that has no attention-map capture.  vep_ok: the caller handles a vep
        model (the forward itself, and variant_prediction_with_attention); predict_step_with_attention does not: it returns
        predict_step's dict."""
        if self.vep and not vep_ok:
            raise NotImplementedError("attention maps: vep models (the ref / het / hom path) are not supported by "
                                      "predict_step_with_attention; variant_prediction_with_attention returns their maps")
        off = [name for name, on in (("only_cross_attention", self.only_cross_attention), ("use_res", self.use_res),
                                     ("cross_alibi", self.cross_alibi), ("add_context_to_cres", self.add_context_to_cres),
                                     (f"gene_pooling={self.gene_pooling!r}", self.gene_pooling != "multi_registry")) if on]
        if off:
            raise NotImplementedError("attention maps: not supported with " + ", ".join(off) + " (the per-(gene, tissue) "
                                      "evaluation order of the options the shipped configuration leaves off)")

    def predict_step_with_attention(self, batch, batch_idx, dataloader_idx=None, layers=None, per_head=False, gene_body=False,
                                    contributions=False, gene_contributions=False, top_k=None):
        """predict_step's dict plus the attention maps of the registry tokens in the same forward:
          "cre_attention"         per gene, fp32 numpy [len(layers), T_i, N_i] -- the head mean of the softmax of gene layer
                                  `layers[k]`'s cross attention on the registry-token row of tissue t (tissues in the order of
                                  tissue_context[i], cCREs in the order of cre_sequences[i]) -- or [len(layers), T_i, H, N_i]
                                  with per_head;
          "cre_attention_layers"  the captured gene-layer indices;
          "gene_attention"        with gene_body: per gene, fp32 numpy [len(layers), T_i, 1 + C_i] ([len(layers), T_i, H, 1 + C_i]
                                  with per_head) -- the same rows' SELF attention (ALiBi, the token at position 0): column 0 is
                                  the registry token itself, column 1 + c gene-body chunk c in the order of gene_embeddings[i].
          "cre_contribution"      with contributions: per gene, fp32 numpy shaped like "cre_attention" -- the norm of the vector
                                  that cCRE j adds to the registry token through the cross attention's out_proj,
                                  || sum_h P[h, j] Wo_h v[j, h] || (per_head: P[h, j] || Wo_h v[j, h] ||, head h's own share):
                                  what the token received, where "cre_attention" says where it looked.  Predictions and the
                                  maps keep their bits with it.
          "gene_contribution"     with gene_contributions (with or without gene_body): per gene, fp32 numpy shaped like
                                  "gene_attention" -- the same norm for the SELF attention's out_proj: column 0 is what the
                                  token's own value adds to it, column 1 + c what gene-body chunk c adds.  ALiBi hands nearby
                                  chunks weight whatever their values are; this is the quantity to rank chunks by, and the one
                                  comparable with "cre_contribution".  Everything else keeps its bits with it.
        layers: distinct gene-layer indices (negative: from the end; None: all; ValueError for an index out of range, an empty
        list or a layer named twice).  When the batch trips the LayerNorm-fold alert the
        recomputation runs under the capture too and the maps are its maps.  A vep model has
        variant_prediction_with_attention instead (variant_prediction's dict plus the same maps).
        top_k: None, or K in 1 .. 64 (ValueError otherwise): the ranking instead of the maps.  The forward and the capture run
        as without it; every requested map is then ranked per row on the device (ops.topk_rows) and only the selections are
        copied to the host.  The four full-map keys above are absent; for each requested map the dict holds
          "<name>_top_value"      per gene, fp32 numpy [len(layers), T_i, K] ([len(layers), T_i, H, K] with per_head): the K
                                  largest entries of the map's row, descending (a NaN first; ties to the lower column);
          "<name>_top_index"      int32, the same shape: their columns in the full map -- cCRE j in the order of
                                  cre_sequences[i]; for the gene-body maps 0 the token itself and 1 + c chunk c -- and -1
                                  (value 0.0) past the gene's last column where it has fewer than K;
          "cre_map_width"         per gene, N_i: how many columns the ranked cCRE maps had ("gene_map_width": 1 + C_i, with
                                  gene_body or gene_contributions).
        A map wider than 16384 columns raises ValueError."""
        self.eval()
        self._attention_maps_supported()
        sel = attn_maps.select_layers(len(self.combined_modulator.gene_layers), layers)
        top_k = attn_maps.select_top_k(top_k)
        with torch.no_grad(), attn_maps.capture(sel, per_head, gene_body, contributions, gene_contributions) as cap:
            out = self.predict_finish(self.predict_launch(self.prepare_batch(batch)), batch_idx, dataloader_idx)
            return self._with_attention(out, cap, top_k)  # the recomputation's maps when predict_finish healed the batch

    def variant_prediction_with_attention(self, batch, layers=None, per_head=False, gene_body=False, contributions=False,
                                          gene_contributions=False, top_k=None):
        """variant_prediction's dict (bit for bit) plus "cre_attention", "cre_attention_layers" and, with gene_body /
        contributions / gene_contributions, "gene_attention" / "cre_contribution" / "gene_contribution" as
        predict_step_with_attention describes them, with one entry per
        genotype of the batch, in batch order: ref, het, hom -- how a variant moved the model's attention.  The VEP forward keeps the full last gene layer (it
        reads token-position rows of it), so every layer records through the row map of the registry rows.  When the batch
        trips the LayerNorm-fold alert the recomputation runs under the capture too and the maps are its maps.
        top_k: as in predict_step_with_attention, one "<name>_top_value" / "<name>_top_index" entry per genotype."""
        self.eval()
        self._attention_maps_supported(vep_ok=True)
        sel = attn_maps.select_layers(len(self.combined_modulator.gene_layers), layers)
        top_k = attn_maps.select_top_k(top_k)
        with torch.no_grad(), attn_maps.capture(sel, per_head, gene_body, contributions, gene_contributions) as cap:
            return self._with_attention(self.variant_prediction(batch), cap, top_k)

    def _with_attention(self, out: dict, cap, top_k=None) -> dict:
        """`out` plus the maps of the capture's most recent forward (call inside the capture block), split per gene; with
        top_k their rankings instead (_with_top_k)."""
        if top_k is not None:
            return self._with_top_k(out, cap, top_k)
        sel, per_head = list(cap.layers), cap.per_head
        H = self.combined_modulator.num_heads

        def per_gene(m, widths):
            if m is None:                                 # no forward ran: an empty batch
                return []
            m = m.detach().cpu().numpy()
            res, r = [], 0
            for t, w in zip(cap.shape[0], widths):
                if per_head:
                    res.append(np.ascontiguousarray(m[:, r * H:(r + t) * H, :w].reshape(len(sel), t, H, w)))
                else:
                    res.append(np.ascontiguousarray(m[:, r:r + t, :w]))
                r += t
            return res
        out["cre_attention"] = per_gene(cap.maps, cap.shape[1] if cap.shape else [])
        out["cre_attention_layers"] = sel
        if cap.gene_body:
            out["gene_attention"] = per_gene(cap.gene_maps, [1 + c for c in cap.shape[2]] if cap.shape else [])
        if cap.contributions:
            out["cre_contribution"] = per_gene(cap.contrib, cap.shape[1] if cap.shape else [])
        if cap.gene_contributions:
            out["gene_contribution"] = per_gene(cap.gene_contrib, [1 + c for c in cap.shape[2]] if cap.shape else [])
        return out

    def _with_top_k(self, out: dict, cap, top_k: int) -> dict:
        """`out` plus, for every map the capture holds, the top_k first-ranked entries of each row and their columns, split per
        gene: each buffer [L, rows, max_k] is ranked as [L * rows, max_k] by one ops.topk_rows call behind the forward, with
        the gene's own width as the row's length (the padding columns are never read), and only the selections are copied."""
        sel, per_head = list(cap.layers), cap.per_head
        H = self.combined_modulator.num_heads
        rep = H if per_head else 1
        tissues = list(cap.shape[0]) if cap.shape else []
        row_len = {}                                      # "cre" / "gene" -> int32 [L * rows] on the device, once per forward

        def lengths(kind, device):
            if kind not in row_len:
                widths = cap.shape[1] if kind == "cre" else [1 + c for c in cap.shape[2]]
                per_row = [int(w) for t, w in zip(tissues, widths) for _ in range(t * rep)]
                row_len[kind] = torch.tensor(per_row * len(sel), dtype=torch.int32).to(device)
            return row_len[kind]

        def ranked(name, m, kind):
            if m is None:                                 # no forward ran: an empty batch
                out[name + "_top_value"], out[name + "_top_index"] = [], []
                return
            if m.shape[-1] > attn_maps.TOP_K_MAX_WIDTH:
                raise ValueError(f"attention maps: top_k ranks maps of at most {attn_maps.TOP_K_MAX_WIDTH} columns, "
                                 f"{name} has {m.shape[-1]}")
            rows = m.shape[0] * m.shape[1]
            assert m.is_contiguous() and m.shape[0] == len(sel) and m.shape[1] == sum(tissues) * rep
            values = torch.empty((rows, top_k), dtype=torch.float32, device=m.device)
            indices = torch.empty((rows, top_k), dtype=torch.int32, device=m.device)
            ops.topk_rows(m.view(rows, m.shape[-1]), top_k, row_len=lengths(kind, m.device), values=values, indices=indices,
                          family=name + "_topk")
            for suffix, buf in (("_top_value", values), ("_top_index", indices)):
                a = buf.cpu().numpy().reshape(len(sel), m.shape[1], top_k)
                res, r = [], 0
                for t in tissues:
                    g = np.ascontiguousarray(a[:, r * rep:(r + t) * rep])
                    res.append(g.reshape(len(sel), t, H, top_k) if per_head else g)
                    r += t
                out[name + suffix] = res
        ranked("cre_attention", cap.maps, "cre")
        out["cre_attention_layers"] = sel
        out["cre_map_width"] = [int(w) for w in cap.shape[1]] if cap.shape else []        # what an index counts up to, per gene
        if cap.gene_body or cap.gene_contributions:
            out["gene_map_width"] = [1 + int(c) for c in cap.shape[2]] if cap.shape else []
        if cap.gene_body:
            ranked("gene_attention", cap.gene_maps, "gene")
        if cap.contributions:
            ranked("cre_contribution", cap.contrib, "cre")
        if cap.gene_contributions:
            ranked("gene_contribution", cap.gene_contrib, "gene")
        return out

    def predict_launch(self, pb: PreparedBatch) -> PredictHandle:
        """Enqueue the forward of a prepared batch; returns without waiting for the GPU (the kernels run on the
        current stream).  `predict_finish` turns the (opaque) handle into predict_step's dict.  Splitting the step lets a
        driver build the next batch on the host while this one computes (processors/trainer.py); any pipelining depth
        is fine: the batch's LayerNorm-fold alert is cut out of the stream's flag right here, behind its last kernel."""
        dev = pb.cre_ids.device
        with torch.no_grad():
            ops.ln_fold_alert_clear(dev)
            pred, emb = self.forward_prepared(pb)
            alert = ops.ln_fold_alert_take(dev)
        done = None
        if dev.type == "cuda":
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))
        return PredictHandle(pb.tissues, pred, emb, self, pb, alert, done)

    @staticmethod
    def predict_finish(handle: PredictHandle, batch_idx, dataloader_idx=None):
        tissues, model, pb = handle.tissues, handle.model, handle.pb
        if handle.done is not None:
            handle.done.synchronize()                        # the launch may have been enqueued on another stream

        def d2h(pe):
            return pe[0].detach().cpu().float().numpy(), pe[1].detach().cpu().float().numpy()
        pred, emb = d2h((handle.pred, handle.emb))           # D2H: the sync point of the step

        def recompute():
            with torch.no_grad():
                return d2h(model.forward_prepared(pb))
        healed = _heal_if_ln_fold_alert(handle.alert, recompute, heal_state(model))
        if healed is not None:
            pred, emb = healed
        preds, embs, s = [], [], 0
        for t in tissues:
            preds.append(pred[s:s + len(t)])
            embs.append(emb[s:s + len(t)])
            s += len(t)
        return {"pred_gene_exp": preds, "embeddings": embs, "batch_idx": batch_idx, "dataloader_idx": dataloader_idx}

    def variant_prediction(self, batch):
        """Reference :909-1004 (VEP: ref / het / hom genotypes, one forward each, plus the embeddings at the
        variant's CRE index and gene-chunk index)."""
        x = batch["cre_sequences"]
        num_batch = len(x)
        if num_batch == 0:
            return {"pred_gene_exp": [], "embd": [], "variant_type": batch["variant_type"],
                    "gene_token_embedding": [], "cre_token_embedding": []}
        cre_pos, gene_pos = batch["cre_token_position"], batch["gene_token_position"]
        assert len(cre_pos) == 3, "there should be 3 samples in the batch for ref, het, hom"
        assert len(gene_pos) == 3, "there should be 3 samples in the batch for ref, het, hom"
        if torch.isnan(torch.as_tensor(cre_pos, dtype=torch.float32)).any():
            cre_pos = None
        if torch.isnan(torch.as_tensor(gene_pos, dtype=torch.float32)).any():
            gene_pos = None
        def run():
            with torch.no_grad():
                pred, _, embd, gtok, ctok = self(
                    x, batch["cre_attention_masks"], batch["tissue_context"], batch["ref_labels"], batch["strand"],
                    batch["gene_embeddings"], batch["gene_attention_masks"], return_embedding=True,
                    cre_token_position=cre_pos, gene_token_position=gene_pos, dedupe_windows=True)
            alert = ops.ln_fold_alert_take(pred.device)       # this batch's bits, behind its last kernel
            return (alert, pred.cpu().float().numpy(), embd.cpu().float().numpy(), gtok.cpu().float().numpy(),
                    ctok.cpu().float().numpy())
        ops.ln_fold_alert_clear(self.device)
        alert, pred, embd, gtok, ctok = run()
        healed = _heal_if_ln_fold_alert(alert, run, heal_state(self))
        if healed is not None:
            _, pred, embd, gtok, ctok = healed
        out = {"pred_gene_exp": [], "embd": [], "variant_type": batch["variant_type"],
               "gene_token_embedding": [], "cre_token_embedding": []}
        s = 0
        for i in range(num_batch):
            n = len(batch["tissue_context"][i])
            out["pred_gene_exp"].append(pred[s:s + n])
            out["embd"].append(embd[s:s + n])
            out["gene_token_embedding"].append(gtok[s:s + n])
            out["cre_token_embedding"].append(ctok[s:s + n])
            s += n
        return out
