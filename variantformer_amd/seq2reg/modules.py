"""seq2reg transformer layer on the HIP kernels (reference: seq2reg/modules.py:129-191)."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops, weights
from ..seq2gene.modules.layers import (MHA, _as_tensor, _cu_from_padded, feed_forward, get_alibi_slopes,  # noqa: F401
                                       layer_streams, packed_linear, pad_input, unpad_input)


class FlashTransformerLayer(nn.Module):
    """LN1 -> self-MHA (ALiBi iff configured) -> +src -> LN2 -> GeGLU(d -> 2048 -> 1024 -> d) -> +src
    (seq2reg/modules.py:149-191; both residuals add the layer INPUT, :152-153,179,188).

    The reference re-pads after attention and zeroes the padded rows (:171-178); pads never feed a valid
    token (attention is varlen, the rest is per-token) and are dropped by the pooling mask, so this
    implementation keeps the stream packed from the embedding to the pool."""

    def __init__(self, d_model, nhead, hidden_dim=2048, dropout=0.1, use_alibi=False, mlp_dout=0.1):
        super().__init__()
        self.MHA = MHA(d_model, nhead, dropout=dropout, use_flash_attn=True, use_alibi=use_alibi)
        self.MHA.family = "seq2reg_self"
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.linear_geglu_1 = nn.Linear(d_model, hidden_dim)
        self.dropout = nn.Dropout(mlp_dout)
        self.linear_geglu_2 = nn.Linear(hidden_dim // 2, d_model)

    def _pooled_down_projection(self, hg, w2, b2, cu, res_f32=None, res16=None, res16_scale: float = 1.0):
        """mean over each window's tokens of (src + linear_geglu_2(hg)) evaluated as mean(src) + W2 mean(hg) + b: the pool
        (seq2reg/model.py:263-267) is linear and so is the layer's last operation (seq2reg/modules.py:184-188), so the
        down-projection runs on W pooled rows instead of n_tok token rows and the fp32 token rows of the encoder output are
        never written.  mean(hg) stays fp32-accurate through the 16-bit GEMM as [hi | lo] against [W2 | W2]; the residual
        mean is taken over the very values the token-level epilogue adds: the fp32 rows, or a 16-bit copy times its scale
        (res16: the fp16 trunk copy, or the operand-type copy of the layer input).  -> fp32 [W, d]."""
        # keyed on the MASTER parameter (as packed_linear is): the packed copy's address can be reused by its successor
        w2_split = weights.derived(self, "_vf_w2_split", (self.linear_geglu_2.weight,),
                                   lambda: torch.cat([w2, w2], dim=1).contiguous())
        ph = ops.segment_mean16(hg, cu, split=True)
        pr = ops.segment_mean16(res16, cu, in_scale=res16_scale) if res16 is not None else \
            ops.segment_mean(res_f32, cu, torch.float32)
        return ops.gemm(ph, w2_split, b2, ops.EPI_RES_F32, residual=pr, family="seq2reg")

    def forward_packed(self, src, cu: torch.Tensor, max_seqlen: int, last: bool = False, keep_x: bool = True,
                       pool_mean: bool = False, qkv: tuple | None = None):
        """src: fp32 [tokens, d] or an ops.LnStream; returns the same kind (an LnStream when LayerNorm is folded into
        the GEMMs, see seq2gene.modules.layers.ln_fold_enabled; a plain tensor from the `last` layer).  keep_x=False: the
        result's fp32 rows have no reader (16-bit trunk, layers.trunk16_enabled) and are not stored.
        pool_mean (with last): return the per-window MEAN of the layer's output rows, fp32 [W, d], instead of the rows
        (_pooled_down_projection).  qkv (folded path): this layer's MHA.project_qkv projection of norm1(src), already made
        (the encoder's first layer looks it up per distinct input row: (table, row per token) of Seq2RegPredictor._layer0_qkv_table)."""
        s = layer_streams(self, src)[0]
        # (folded, x1 is read only through norm2 -> linear_geglu_1: no fp32 store, and its residual is the 16-bit copy of the input)
        x1 = self.MHA.self_block(s, self.norm1, cu, max_seqlen, qkv=qkv)
        if last and pool_mean:
            return feed_forward(x1, self.norm2, self, s,
                                pooled=lambda hg, w2, b2, **res: self._pooled_down_projection(hg, w2, b2, cu, **res))
        # the encoder's last layer feeds the pooling, not a LayerNorm: plain fp32 rows.  Otherwise, 16-bit trunk
        # (layers.trunk16_enabled): the next layer reads the 16-bit copies + statistics only
        return feed_forward(x1, self.norm2, self, s, keep_x=keep_x, rows32=last)

    def forward(self, src, src_key_padding_mask=None, precision=torch.float32):
        """Reference signature on padded [b, L, d] input; padded rows of the result are left as the
        reference leaves them only where they matter (valid rows); pad rows are returned as zeros."""
        b, L = src.shape[:2]
        if src_key_padding_mask is None:
            out = _as_tensor(self.forward_packed(src.reshape(b * L, -1).float().contiguous(), _cu_from_padded(b, L, src.device), L))
            return out.view(b, L, -1).to(src.dtype)
        xs, idx, cu, mx, _ = unpad_input(src, ~src_key_padding_mask)
        return pad_input(_as_tensor(self.forward_packed(xs, cu, mx)), idx, b, L).to(src.dtype)
