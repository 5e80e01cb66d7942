"""GRL-B x4 on the HIP kernels (host side).  Mirrors src/models/grl/grl_arch.py (GRL.forward :506,
forward_features :494, TransformerStage.forward :168) and grl/common/mixed_attn_block_efficient.py
(MixedAttention.forward :348, EfficientMixAttnTransformerBlock.forward :537).

Host-side fixes of the reference's hidden costs: the CPB-MLP position bias
(AffineTransform, :36-47) is input independent, so it is evaluated ONCE at load time per block instead
of 120x per forward; shift masks are computed inside the attention kernel from region ids instead of
being rebuilt on the CPU and copied per image (grl_arch.py:431-453).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import ops
from .common import CAB, SRTail, dev, to_map, tokens
from .ops import ACT_GELU

WS, DF = 8, 2


def _coords_table(ws, aws):
    hi = ws - 1 - (ws - aws) // 2
    lo = -(aws - 1) - (ws - aws) // 2
    c = torch.arange(lo, hi + 1, dtype=torch.float32)
    t = torch.stack(torch.meshgrid(c, c, indexing="ij"), -1) / hi * 8
    return torch.sign(t) * torch.log2(t.abs() + 1.0) / math.log2(8)


def _rel_index(ws, aws, window_to_anchor):
    def grid(n):
        return torch.stack(torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")).flatten(1)
    cw, ca = grid(ws), grid(aws)
    span = aws + ws - 1
    d = (cw[:, :, None] - ca[:, None, :]) + (aws - 1) if window_to_anchor else (ca[:, :, None] - cw[:, None, :]) + (ws - 1)
    return d[0] * span + d[1]


def _cpb_bias_T(sd, p, table, index, device):
    """16 * sigmoid(CPB_MLP(table))[index] as [heads, N_keys, N_queries] (transposed for lane-coalesced reads)
    plus exp(min(logit_scale, ln 100)) per head.  Weight pre-processing (input independent), done on the host."""
    # (the tables are built on the host: the few KB of CPB-MLP weights come to the CPU wherever the state_dict lives)
    h = F.relu(F.linear(table.reshape(-1, 2), sd[p + "cpb_mlp.0.weight"].float().cpu(), sd[p + "cpb_mlp.0.bias"].float().cpu()))
    tab = F.linear(h, sd[p + "cpb_mlp.2.weight"].float().cpu())
    b = 16 * torch.sigmoid(tab[index.reshape(-1)].reshape(index.shape[0], index.shape[1], -1))   # [Nq, Nk, heads]
    logit = torch.clamp(sd[p + "logit_scale"].float().cpu().reshape(-1), max=math.log(100.0)).exp()
    return dev(b.permute(2, 1, 0), device), dev(logit, device)


class _Block:
    def __init__(self, sd, p, device, dim, heads, window_shift):
        self.dim, self.heads, self.hd = dim, heads, dim // 2 // heads
        self.shift = WS // 2 if window_shift else 0
        a = p + "attn."
        self.qkv = ops.pack_conv(sd[a + "qkv.body.weight"], sd[a + "qkv.body.bias"], device)
        # qkv on the token GEMM (rows in registers, no LayerNorm: GRL is post-norm) instead of the planes tile kernel
        self.qkv_t = ops.pack_tok_gemm(sd[a + "qkv.body.weight"], sd[a + "qkv.body.bias"], device) \
            if ops.tok_gemm_ok(dim, 3 * dim) else None
        self.anchor = ops.pack_conv(sd[a + "anchor.body.0.reduction.weight"], sd[a + "anchor.body.0.reduction.bias"], device)
        self.proj = ops.pack_conv(sd[a + "proj.weight"], sd[a + "proj.bias"], device)
        AW = WS // DF
        self.bw, self.lw = _cpb_bias_T(sd, a + "window_attn.attn_transform.", _coords_table(WS, WS),
                                       _rel_index(WS, WS, True), device)
        tab = _coords_table(WS, AW)
        self.b1, self.l1 = _cpb_bias_T(sd, a + "stripe_attn.attn_transform1.", tab, _rel_index(WS, AW, False), device)
        self.b2, self.l2 = _cpb_bias_T(sd, a + "stripe_attn.attn_transform2.", tab, _rel_index(WS, AW, True), device)
        self.n1 = (dev(sd[p + "norm1.weight"], device), dev(sd[p + "norm1.bias"], device))
        self.n2 = (dev(sd[p + "norm2.weight"], device), dev(sd[p + "norm2.bias"], device))
        self.cab = CAB(sd, p + "conv.", device)
        self.fc1 = ops.pack_conv(sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], device)
        self.fc2 = ops.pack_conv(sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"], device)
        # y + norm2(mlp(y)) as ONE kernel (fc1, GELU, fc2, LayerNorm of the output row, residual; fp32 + planes out)
        self.mlp = ops.pack_tok_chain(sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], sd[p + "mlp.fc2.weight"],
                                      sd[p + "mlp.fc2.bias"], device, mode=0) if ops.tok_chain_ok(dim, dim, 0) else None
        # ... with the attention's output projection, norm1 and the two residuals as its head (x + norm1(proj(attn)) + CAB(x) stays
        # in the kernel's registers): mixed_attn_block_efficient.py:536-554
        self.proj_t = ops.pack_tok_gemm(sd[a + "proj.weight"], sd[a + "proj.bias"], device) \
            if self.mlp is not None and ops.tok_gemm_ok(dim, dim) and ops.tok_head_ok(dim, "post") else None

    def __call__(self, x, B, H, W, xp=None):
        """x [P, dim] contiguous tokens (xp: the same tensor as bf16 hi/lo planes, if the producer emitted them)
        -> ([P, dim], planes of it or None)"""
        C, hd, heads = self.dim, self.hd, self.heads
        split = ops.split_mode()
        xm = to_map(x, B, H, W)
        if self.qkv_t is not None and split:
            qkv = ops.tok_gemm(x, self.qkv_t)                              # [P, 3C]: window half | stripe half
        else:
            qkv = ops.linear(xp if xp is not None else x, self.qkv)
        anchor = ops.conv2d(ops.avgpool2(xm), self.anchor)                # [B, H/2, W/2, C/2]
        cat = torch.empty(x.shape[0], C, device=x.device)
        ops.grl_window_attn(qkv, 0, self.bw, self.lw, cat, 0, B, H, W, heads, hd, self.shift)
        ops.grl_stripe_attn(qkv, 3 * C // 2, anchor, self.b1, self.b2, self.l1, self.l2, cat, C // 2, B, H, W, heads, hd)
        c2, att = self.cab(xp.reshape_map(B, H, W) if xp is not None else xm)
        if self.proj_t is not None and split:
            return ops.tok_head_chain(cat, self.proj_t, self.mlp, head_ln=self.n1, hres=x, hres2=tokens(c2), hvec2=att,
                                      rows_per_batch=H * W, post_ln=self.n2, out_planes=True)
        a = ops.linear(cat, self.proj)
        # y = x + LN(attn(x)) + CAB(x): the channel-attention scaling of CAB (c2 * att[batch]) rides in the LN kernel
        if not split:
            y = ops.layernorm(a, *self.n1, res1=x, res2=tokens(c2), res2_vec=att, rows_per_batch=H * W)
            m = ops.linear(ops.linear(y, self.fc1, act=ACT_GELU), self.fc2)
            return ops.layernorm(m, *self.n2, res1=y), None
        # split mode, a width without the head kernel (tok_head_ok) or without an MLP kernel
        if self.mlp is not None:
            y = ops.layernorm(a, *self.n1, res1=x, res2=tokens(c2), res2_vec=att, rows_per_batch=H * W)
            return ops.tok_chain(y, self.mlp, post_ln=self.n2, res2=y, out_planes=True)
        y, yp = ops.layernorm(a, *self.n1, res1=x, res2=tokens(c2), res2_vec=att, rows_per_batch=H * W, out_planes=True)
        m = ops.linear(ops.linear(yp, self.fc1, act=ACT_GELU, out_planes=True, want_f32=False), self.fc2)
        return ops.layernorm(m, *self.n2, res1=y, out_planes=True)


class GRL:
    def __init__(self, sd, device, heads=3):
        self.device = device
        self.embed = sd["conv_first.weight"].shape[0]
        depths = {}
        for k in sd:
            if k.startswith("layers.") and ".blocks." in k:
                parts = k.split(".")
                depths[int(parts[1])] = max(depths.get(int(parts[1]), 0), int(parts[3]) + 1)
        self.conv_first = ops.pack_conv(sd["conv_first.weight"], sd["conv_first.bias"], device)
        self.norm_start = (dev(sd["norm_start.weight"], device), dev(sd["norm_start.bias"], device))
        self.norm_end = (dev(sd["norm_end.weight"], device), dev(sd["norm_end.bias"], device))
        self.stages = []
        for i in sorted(depths):
            blocks = [_Block(sd, f"layers.{i}.blocks.{j}.", device, self.embed, heads, window_shift=(j % 2 == 0))
                      for j in range(depths[i])]
            conv = ops.pack_conv(sd[f"layers.{i}.conv.weight"], sd[f"layers.{i}.conv.bias"], device)
            self.stages.append((blocks, conv))
        self.tail = SRTail(sd, device, up_prefix="upsample.up.")

    def __call__(self, lr):
        """lr [B,H,W,3] (H, W multiples of 8) -> (sr un-clamped [B,4H,4W,3], feat [B,H,W,embed])."""
        B, H, W, _ = lr.shape
        if H % WS or W % WS:
            raise ValueError(f"GRL input {H}x{W} must be a multiple of {WS}")
        x0 = ops.conv2d(self.tail.center(lr), self.conv_first)
        t = ops.layernorm(tokens(x0), *self.norm_start)
        for blocks, conv in self.stages:
            r, rp = t, None
            for blk in blocks:
                r, rp = blk(r, B, H, W, rp)
            src = rp.reshape_map(B, H, W) if rp is not None else to_map(r, B, H, W)
            t = tokens(ops.conv2d(src, conv, res=to_map(t, B, H, W)))
        return self.tail(ops.final_norm(t, self.norm_end, B, H, W), x0)
