"""Executor of the plain (non-residual) U-Net, 2D and 3D, on the MI355X kernels (SURVEY.md row U / cfg 1 family).

Host side of biapy/models/unet.py:382-420 and of its autograd graph, built from the same C-ABI kernels as the residual
network (engine.py) plus the materialised InstanceNorm+activation pair (``bpx_norm_act_fwd`` / ``bpx_norm_act_bwd``):

  * inside a ConvBlock (blocks.py:120-167, ``nconvs`` x [Conv -> IN -> act]) the normalisation + activation between two
    convolutions never materialises: the consumer conv applies the producer's (mean, rstd, scale, shift) records while
    staging its halo, exactly as in the residual network;
  * the block OUTPUT ``act(IN(conv))`` feeds MaxPool / ConvTranspose / the head / the skip connection, none of which has a
    fused prologue, so it is written once by ``bpx_norm_act_fwd`` - the skip copy straight into the channel slice
    ``[Cup, Cup+Cskip)`` of the level's concat buffer (``torch.cat([up, bridge], 1)``, blocks.py:666, is a layout decision);
  * ``UpBlock.up`` = ConvTranspose(in -> out) -> IN -> act (blocks.py:602-614): raw transposed-conv output + statistics, then
    ``bpx_norm_act_fwd`` into channels ``[0, Cup)`` of the concat buffer.

2D networks run as 3D tensors with one z-slice: (B,C,Y,X) <-> NDHWC with D = 1, 3x3 kernels zero-padded to 3x3x3
(only the centre z-tap is non-zero), pooling / transposed convolutions with the (1,2,2) variants.  That wastes 2/3 of the
MFMA work of those layers; cfg 1 is the reference's CPU plumbing configuration, a parity case and not a bench line.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import copy

import torch

from . import _lib as L
from .engine import NetConfig, ResUNetEngine, _Stats, lift_params, pad_input_channels, unlift_grads, unpad_input_grads

lib = L.lib


@dataclass
class _CB:
    """What the backward needs about one ConvBlock (two convolutions)."""
    prefix: str
    S: Tuple[int, int, int]
    cin: int
    cout: int
    x: Optional[torch.Tensor]          # materialised block input (None: the 1-channel image)
    h: List[torch.Tensor]              # raw conv outputs
    rec: List[torch.Tensor]            # their norm records


class UNetEngine(ResUNetEngine):
    _unet_layout = True

    def __init__(self, cfg: NetConfig, ndim: int, dtype: torch.dtype = torch.bfloat16, nconvs: int = 2):
        super().__init__(cfg, dtype)
        assert ndim in (2, 3)
        if nconvs != 2:
            raise NotImplementedError("UNetEngine: conv_layers must be 2 at every level")
        self.ndim = ndim
        self.nconvs = nconvs
        if cfg.gn_groups:
            # unet.U_Net builds InstanceNorm layers whatever `normalization` names, and this engine has always run them as such: the shared norm
            # helpers (_norm_records, _norm_bwd_coef) read the group count from the configuration
            self.cfg = copy.copy(cfg)
            self.cfg.gn_groups = 0

    # ---- parameters: 2D weights are lifted to one-z-slice 3D weights (engine.lift_params); the first convolution of a network whose image is
    # zero-padded to 16 channels (NetConfig.true_in_ch) gets zero input-channel columns (engine.pad_input_channels) ------------------------
    def _lift(self, P: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        if self.cfg.true_in_ch is not None:
            P = pad_input_channels(P, self.cfg.in_ch)
        return lift_params(P) if self.ndim == 2 else P

    # ---- forward ------------------------------------------------------------------------------------------------------
    def _conv_block_fwd(self, P, prefix, B, S, cin, cout, x, img, out_view, st, dev) -> _CB:
        D, H, W = S
        vox = D * H * W
        T = self.dtype
        cb = _CB(prefix, S, cin, cout, x, [], [])
        src, src_rec = x, None
        for c in range(self.nconvs):
            kw, kb = f"{prefix}.block.{c}.block.0.weight", f"{prefix}.block.{c}.block.0.bias"
            h = torch.empty((B, D, H, W, cout), dtype=T, device=dev)
            if c == 0 and img is not None:
                tiles = lib.bpx_conv3d_c1_stats_tiles(D, H, W)
                part = _Stats.alloc(B, tiles, cout, dev)
                L.check(lib.bpx_conv3d_c1_fwd(self.dt, B, D, H, W, img.data_ptr(), P[kw].data_ptr(), P[kb].data_ptr(), L.tview(h), part.data_ptr(), st))
            else:
                ci = cin if c == 0 else cout
                tiles = lib.bpx_conv3d_stats_tiles(self.dt, B, D, H, W, cout)
                part = _Stats.alloc(B, tiles, cout, dev)
                wp = self._pack(P[kw], L.PK_K3, ci, cout, False)
                L.check(lib.bpx_conv3d_fwd(self.dt, B, D, H, W, L.tview(src), L.ptr(src_rec), self.act if src_rec is not None else 0,
                                           wp.data_ptr(), P[kb].data_ptr(), L.NULL_T, None, None, L.tview(h), part.data_ptr(), st))
            rec = self._norm_records(P, f"{prefix}.block.{c}.block.1", part, tiles, cout, vox, st)
            cb.h.append(h)
            cb.rec.append(rec)
            src, src_rec = h, rec
        L.check(lib.bpx_norm_act_fwd(self.dt, B, vox, L.tview(src), src_rec.data_ptr(), self.act, out_view, st))
        return cb

    def forward(self, P: Dict[str, torch.Tensor], x: torch.Tensor, head_act: int = 0, save: bool = False, cache_weights: bool = False):
        """x: (B,C,Y,X) [2D] or (B,C,Z,Y,X) [3D] fp32.  Returns logits in the same channels-first planar layout, and the context."""
        cfg = self.cfg
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == self.ndim + 2
        groups = self._groups_for(x.shape[0], ((1,) + tuple(x.shape[2:]))[-3:], save)
        if len(groups) > 1:
            return self._forward_groups(groups, lambda **a: self.forward(P, head_act=head_act, cache_weights=cache_weights, **a), x, save)
        if self.ndim == 2:
            x = x.unsqueeze(2)
        B, Cin, D0, H0, W0 = x.shape
        assert Cin == (cfg.true_in_ch or cfg.in_ch), f"expected {cfg.true_in_ch or cfg.in_ch} input channels, got {Cin}"
        Lv = cfg.depth
        zd = cfg.z_down if self.ndim == 3 else (1,) * Lv
        S = self._level_shapes((D0, H0, W0), zd)
        dev, st, T = x.device, L.stream_ptr(), self.dtype
        fm = list(cfg.feature_maps)
        self._prepacked = {}
        Pw = self._lift(P)
        img, cur = self._ingest(x, None, st)

        def buf(i, C):
            return torch.empty((B,) + S[i] + (C,), dtype=T, device=dev)

        cat = [buf(i, 2 * fm[i]) for i in range(Lv)]           # [up (fm[i]) | skip (fm[i])]
        blocks: List[_CB] = []
        # ---------------- encoder ------------------------------------------------------------------
        for i in range(Lv):
            cin = cfg.in_ch if i == 0 else fm[i - 1]
            cb = self._conv_block_fwd(Pw, f"down_path.{i}", B, S[i], cin, fm[i], cur, img if i == 0 else None, L.tview(cat[i], fm[i], fm[i]), st, dev)
            blocks.append(cb)
            D, H, W = S[i]
            pooled = buf(i + 1, fm[i])
            ppart = _Stats.alloc(B, lib.bpx_maxpool3d_stats_tiles(self.dt, D, H, W, zd[i], fm[i]), fm[i], dev)   # statistics unused here
            L.check(lib.bpx_maxpool3d_fwd(self.dt, B, D, H, W, zd[i], L.tview(cat[i], fm[i], fm[i]), L.tview(pooled), ppart.data_ptr(), st))
            cur = pooled
        # ---------------- bottleneck ----------------------------------------------------------------
        bott = buf(Lv, fm[Lv])
        blocks.append(self._conv_block_fwd(Pw, "bottleneck", B, S[Lv], fm[Lv - 1], fm[Lv], cur, None, L.tview(bott), st, dev))
        # ---------------- decoder -------------------------------------------------------------------
        dec_in, ups = bott, []
        for j, i in enumerate(range(Lv - 1, -1, -1)):
            Cl, Cup = fm[i + 1], fm[i]
            Dl, Hl, Wl = S[i + 1]
            wk, bk = f"up_paths.0.{j}.up.0.weight", f"up_paths.0.{j}.up.0.bias"
            wp = self._pack(Pw[wk], L.PK_CT if zd[i] == 2 else L.PK_CT4, Cl, Cup, False)
            utiles = lib.bpx_convT3d_stats_tiles(Dl, Hl, Wl, zd[i])
            upart = _Stats.alloc(B, utiles, Cup, dev)
            up_raw = buf(i, Cup)
            L.check(lib.bpx_convT3d_k2s2_fwd(self.dt, B, Dl, Hl, Wl, zd[i], L.tview(dec_in), wp.data_ptr(), Pw[bk].data_ptr(), L.tview(up_raw),
                                             upart.data_ptr(), st))
            vox = S[i][0] * S[i][1] * S[i][2]
            urec = self._norm_records(Pw, f"up_paths.0.{j}.up.1", upart, utiles, Cup, vox, st)
            L.check(lib.bpx_norm_act_fwd(self.dt, B, vox, L.tview(up_raw), urec.data_ptr(), self.act, L.tview(cat[i], 0, Cup), st))
            out = buf(i, fm[i])
            blocks.append(self._conv_block_fwd(Pw, f"up_paths.0.{j}.conv_block", B, S[i], 2 * fm[i], fm[i], cat[i], None, L.tview(out), st, dev))
            ups.append((j, i, dec_in, up_raw, urec))
            dec_in = out
        # ---------------- heads ----------------------------------------------------------------------
        hw, hb = self._head_matrix(Pw)
        logits, _ = self._head_fwd(B, S[0], dec_in, hw, hb, head_act, st, dev)
        if self.ndim == 2:
            logits = logits.reshape(B, -1, H0, W0)
        ctx = dict(B=B, S=S, zd=zd, img=img, blocks=blocks, cat=cat, ups=ups, feat=dec_in, hw=hw, Pw=Pw) if save else None
        return logits, ctx

    # ---- backward -------------------------------------------------------------------------------------------------------
    def _conv_block_bwd(self, Pw, G, cb: _CB, B, dA: "L.Tensor", img, dx_out: Optional["L.Tensor"], st, dev):
        D, H, W = cb.S
        vox = D * H * W
        p, C1 = cb.prefix, cb.cout
        k = lambda c, leaf: f"{p}.block.{c}.block.{leaf}"   # noqa: E731
        # output norm+act of the last conv
        g2 = self._norm_act_bwd(cb.h[1], cb.rec[1], self.act, dA, Pw[k(1, "1.weight")], G[k(1, "1.weight")], G[k(1, "1.bias")], st)
        self._keep.append(g2)
        # conv 2: weights, then the input gradient fused with act' and the reductions of the first norm
        self._wgrad(B, cb.S, L.tview(cb.h[0]), cb.rec[0], self.act, L.tview(g2), 3, G[k(1, "0.weight")], G[k(1, "0.bias")], st, dev)
        g1 = torch.empty((B, D, H, W, C1), dtype=self.gdtype, device=dev)
        self._keep.append(g1)
        w2t = self._pack(Pw[k(1, "0.weight")], L.PK_K3_T, C1, C1, False)
        tiles, red = self._dgrad_prologue(B, cb.S, L.tview(g2), w2t, L.tview(cb.h[0]), cb.rec[0], self.act, L.tview(g1), st, fused=False)
        coef = self._norm_bwd_coef(red, B, tiles, C1, vox, cb.rec[0], Pw[k(0, "1.weight")], G[k(0, "1.weight")], G[k(0, "1.bias")], st, deferred=False)
        L.check(lib.bpx_norm_bwd_apply(self.bdt, B, vox, L.tview(g1), L.tview(cb.h[0]), coef.data_ptr(), L.NULL_T, L.tview(g1), st))
        # conv 1
        if img is not None:
            wsc = self._workspace(lib.bpx_conv3d_c1_wgrad_workspace(C1), dev)
            L.check(lib.bpx_conv3d_c1_wgrad(self.gdt, B, D, H, W, img.data_ptr(), L.tview(g1), G[k(0, "0.weight")].data_ptr(),
                                            G[k(0, "0.bias")].data_ptr(), wsc.data_ptr(), wsc.numel(), st))
            return
        self._wgrad(B, cb.S, L.tview(cb.x), None, 0, L.tview(g1), 3, G[k(0, "0.weight")], G[k(0, "0.bias")], st, dev)
        if dx_out is not None:
            w1t = self._pack(Pw[k(0, "0.weight")], L.PK_K3_T, cb.cin, C1, False)
            L.check(lib.bpx_conv3d_dgrad(self.gdt, B, D, H, W, L.tview(g1), w1t.data_ptr(), L.NULL_T, None, 0, dx_out, None, st))

    def backward(self, P: Dict[str, torch.Tensor], ctx, dlogits: torch.Tensor) -> Dict[str, torch.Tensor]:
        if "groups" in ctx:
            return self._backward_groups(ctx, dlogits, lambda c, d: self.backward(P, c, d))
        Pw = ctx["Pw"]
        with self._backward_pass(defer=False):
            G = self._grad_slab(Pw, dlogits.device)        # in the LIFTED shapes, un-lifted at the end
            self._backward(Pw, G, ctx, dlogits)
        if self.cfg.true_in_ch is not None:
            G = unpad_input_grads(G, self.cfg.true_in_ch)
        return unlift_grads(G, P)   # gradients in the shapes of the module's parameters

    def _backward(self, Pw, G, ctx, dlogits: torch.Tensor) -> None:
        cfg = self.cfg
        B, S, zd, img = ctx["B"], ctx["S"], ctx["zd"], ctx["img"]
        blocks: List[_CB] = ctx["blocks"]
        cat, ups, feat = ctx["cat"], ctx["ups"], ctx["feat"]
        fm, Lv = list(cfg.feature_maps), cfg.depth
        dev, st, T = dlogits.device, L.stream_ptr(), self.gdtype       # T: storage type of the gradient tensors
        # ---- head -------------------------------------------------------------------------------
        dl = dlogits.contiguous().float()
        dfeat = torch.empty((B,) + S[0] + (fm[0],), dtype=T, device=dev)
        self._head_bwd(G, B, S[0], L.tview(feat), ctx["hw"], dl, L.tview(dfeat), st, dev)
        # ---- decoder: walk from level 0 down to the bottleneck ---------------------------------------------------------
        dcat: List[Optional[torch.Tensor]] = [None] * Lv
        dA = L.tview(dfeat)
        self._keep.append(dfeat)
        for j, i, x_low, up_raw, urec in reversed(ups):
            Cl, Cup = fm[i + 1], fm[i]
            dcat[i] = torch.empty((B,) + S[i] + (2 * fm[i],), dtype=T, device=dev)
            self._conv_block_bwd(Pw, G, blocks[Lv + 1 + j], B, dA, None, L.tview(dcat[i]), st, dev)
            pre = f"up_paths.0.{j}.up"
            dup = self._norm_act_bwd(up_raw, urec, self.act, L.tview(dcat[i], 0, Cup), Pw[f"{pre}.1.weight"], G[f"{pre}.1.weight"],
                                     G[f"{pre}.1.bias"], st)
            dA = L.tview(self._convT_bwd(Pw, G, B, S[i + 1], zd[i], x_low, dup, f"{pre}.0.weight", f"{pre}.0.bias", Cl, Cup, st, dev))
        # ---- bottleneck ---------------------------------------------------------------------------------------------
        dP = torch.empty((B,) + S[Lv] + (fm[Lv - 1],), dtype=T, device=dev)
        self._conv_block_bwd(Pw, G, blocks[Lv], B, dA, None, L.tview(dP), st, dev)
        # ---- encoder ------------------------------------------------------------------------------------------------
        for i in range(Lv - 1, -1, -1):
            D, H, W = S[i]
            # d(skip output) = d(concat)[..., Cup:] + unpool(dP), in place over the skip slice
            skipv = L.tview(dcat[i], fm[i], fm[i])
            L.check(lib.bpx_maxpool3d_bwd(self.bdt, B, D, H, W, zd[i], L.tview(cat[i], fm[i], fm[i]), L.tview(dP), skipv, skipv, st))
            if i > 0:
                dPn = torch.empty((B,) + S[i] + (fm[i - 1],), dtype=T, device=dev)
                self._conv_block_bwd(Pw, G, blocks[i], B, skipv, None, L.tview(dPn), st, dev)
                self._keep.append(dP)
                dP = dPn
            else:
                self._conv_block_bwd(Pw, G, blocks[0], B, skipv, img, None, st, dev)   # the image needs no gradient
