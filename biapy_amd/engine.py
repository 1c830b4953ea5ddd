"""Executor of the 3D residual U-Net on the MI355X kernels (forward, and the hand-written backward).

This is the host side of biapy/models/resunet.py:352-446 (forward graph) and of the autograd graph
PyTorch would build for it (train_engine.py:173 ``loss.backward()``): it sequences the C-ABI kernels
of include/biapy_amd.h on the current HIP stream.  No arithmetic happens here and no PyTorch operator
touches an activation; PyTorch only owns the memory.

Data layout in HBM (all NDHWC, storage dtype T = bf16 or f32):
  * every raw (pre-normalisation) tensor is written once by its producer and read by its consumers;
    InstanceNorm+ELU never materialise - the producer emits per-(n,c) partial statistics, a tiny
    finalize kernel turns them into (mean, rstd, scale, shift) records and the consumer conv applies
    them while staging its input halo in LDS;
  * torch.cat([up, skip], 1) (blocks.py:1653) is a layout decision, not a kernel: each level owns one
    buffer [B,S,S,S,Cup+Cskip]; the transposed conv writes channels [0,Cup), the encoder block writes
    its output directly into [Cup, Cup+Cskip);
  * the residual add and the 1x1x1 shortcut conv (blocks.py:1372,1458) are extra K-steps of the
    block's second 3x3x3 conv kernel.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import contextlib
import ctypes as C
import math

import torch

from . import _lib as L

lib = L.lib
EPS = 1e-5

# Packed-operand caches are keyed by (storage address, tensor version) - but a HIP-graph replay of an optimizer step rewrites the
# parameters WITHOUT bumping ``_version``.  Every replaying object of this package (graphs.GraphedTrainStep /
# DataParallelTrainStep, train_engine._restore) therefore bumps this process-wide counter, which is part of every cache key.
_WEIGHTS_EPOCH = [0]


def bump_weights_epoch() -> None:
    _WEIGHTS_EPOCH[0] += 1


def weights_epoch() -> int:
    return _WEIGHTS_EPOCH[0]


@dataclass
class NetConfig:
    in_ch: int
    feature_maps: Sequence[int]
    out_channels: Sequence[int] = (1,)
    activation: str = "elu"
    normalization: str = "in"
    z_down: Optional[Sequence[int]] = None    # MODEL.Z_DOWN per level (1 or 2; None = 2 everywhere); YX_DOWN is always 2
    ndim: int = 3                             # 2: (B,C,Y,X) tensors, run as one-z-slice volumes (z_down is then 1 everywhere)
    post_up: int = 0                          # super-resolution "post" up-sampling ConvTranspose3d(fm0, fm0, k = s = (post_up, 2, 2)) in front
    #                                           of the heads (resunet.py:326-333, :399-400); 0 = none, else the z factor (1 or 2)
    dropout: Optional[Sequence[float]] = None # MODEL.DROPOUT_VALUES: one probability per level, the last one for the bottleneck (resunet.py:250, :270, :299); None / 0 = none

    def __post_init__(self):
        fm = list(self.feature_maps)
        zd = [2] * (len(fm) - 1) if self.z_down is None else [int(v) for v in list(self.z_down)[: len(fm) - 1]]
        if len(zd) != len(fm) - 1 or any(v not in (1, 2) for v in zd):
            raise NotImplementedError(f"z_down={self.z_down!r}: one value per level, each 1 or 2")
        self.z_down = tuple(zd)
        if self.normalization not in ("in", "gn", "bn"):
            raise NotImplementedError(f"normalization={self.normalization!r}: the MI355X engine implements 'in' (the reference default), 'gn' and 'bn' "
                                      f"(sync_bn: cross-rank batch statistics are not implemented)")
        if self.normalization == "bn":
            # BatchNorm3d (blocks.py:2113-2127): statistics over the whole batch (bpx_batchnorm_finalize), running buffers on the device
            why = ("2-D networks" if self.ndim != 3 else "feature maps that are not multiples of 16" if any(int(c) % 16 for c in fm)
                   else "super-resolution stages" if self.post_up else "dropout (drop_values > 0)" if self.dropout is not None and any(float(v) > 0 for v in self.dropout)
                   else None)
            if why:
                raise NotImplementedError(f"normalization='bn': {why} are not implemented with BatchNorm on the MI355X engine")
        # 'gn': torch.nn.GroupNorm(8, C) for every norm layer - what blocks.py:2122-2125 means (the reference's own call,
        # nn.GroupNorm(out_channels, num_groups=8), raises a TypeError, so there is no reference output to pin this mode to)
        self.gn_groups = 8 if self.normalization == "gn" else 0
        if self.gn_groups:
            # checked here, not by a kernel in the middle of the first forward: bpx_norm_finalize / bpx_norm_bwd_finalize take
            # 1, 2, 4, ... 64 channels per group for the single-producer tensors; the concatenated decoder inputs (any channels per group) go
            # through the general group kernels, which only need whole groups
            ok_cpg = (1, 2, 4, 8, 16, 32, 64)
            for i, c in enumerate(fm):
                if c % self.gn_groups or (c // self.gn_groups) not in ok_cpg:
                    raise NotImplementedError(f"normalization='gn': feature_maps[{i}] = {c} gives {c / self.gn_groups:g} channels per group; the kernels "
                                              f"take {ok_cpg} (GroupNorm(8, C): C in 8 ... 512, a power of two times 8)")
            for i in range(len(fm) - 1):
                if (fm[i] + fm[i + 1]) % self.gn_groups:
                    raise NotImplementedError(f"normalization='gn': the concatenated decoder input of level {i} has {fm[i] + fm[i + 1]} channels, not a multiple of 8")
        if self.activation not in L.ACT:
            raise NotImplementedError(f"activation={self.activation!r} is not implemented on the MI355X engine")
        # Widths that are not multiples of 16 (e.g. MODEL.FEATURE_MAPS [52, 68, 84] of the reference's CartoCell template) run zero-padded to the next
        # multiple (the MFMA tile): `feature_maps` becomes what the kernels see, `true_feature_maps` what the parameters have.  Exact under InstanceNorm:
        # a padded channel is produced by zero weights and read through zero weights (channel_pad_plan / pad_channels below).
        self.true_feature_maps = None
        if any(c % 16 for c in fm):
            if self.gn_groups or self.post_up or self.in_ch != 1:
                raise NotImplementedError(f"feature_maps {fm} (not multiples of 16) run zero-padded: InstanceNorm, one input channel and no super-resolution stage only")
            self.true_feature_maps = tuple(fm)
            fm = [(c + 15) // 16 * 16 for c in fm]
            self.feature_maps = fm
        # Images of 2 to 15 channels (RGB, two stains, image + prior) run zero-padded to 16 channels, as the widths above do: `in_ch` becomes what
        # the kernels see, `true_in_ch` what the image and the first block's two input weights have (pad_input_channels / unpad_input_grads
        # below; bpx_image_pack16 writes the padded tensor).  Exact: the padded channels are zeros read through zero weight columns.
        self.true_in_ch = None
        if 2 <= self.in_ch <= 15:
            self.true_in_ch, self.in_ch = int(self.in_ch), 16
        elif self.in_ch != 1 and self.in_ch % 16:
            raise NotImplementedError(f"input channels must be 1 to 16 or a multiple of 16 (got {self.in_ch}): only images of up to 15 channels are "
                                      f"zero-padded (to 16)")
        if self.post_up not in (0, 1, 2):
            raise NotImplementedError("post up-sampling: z factor 1 or 2 (y / x factor 2)")
        if sum(self.out_channels) > 8:
            raise NotImplementedError(f"output head supports <= 8 channels (got {sum(self.out_channels)})")
        self.depth = len(fm) - 1
        dv = [0.0] * len(fm) if self.dropout is None else [float(v) for v in list(self.dropout)]
        if len(dv) < len(fm) or any(not (0.0 <= v < 1.0) for v in dv):
            raise ValueError(f"dropout={self.dropout!r}: one probability in [0, 1) per level and one for the bottleneck")
        self.dropout = tuple(dv[: len(fm) - 1]) + (dv[-1],)      # levels 0 .. depth-1, bottleneck (the reference indexes drop_values[i] and [-1])


def set_compute_dtype(model, dtype: torch.dtype) -> torch.dtype:
    """Switch the storage type of a drop-in model (workflow.SlidingWindowPredictor, train_engine.evaluate); returns the previous one.
    Refused up front - not by a kernel in the middle of a predict call - when the model's engine has no kernels for it."""
    ok = getattr(model, "supported_compute_dtypes", (torch.float32, torch.bfloat16))
    if dtype not in ok:
        raise NotImplementedError(f"{type(model).__name__}: compute_dtype={dtype} is not implemented for this model (supported: {', '.join(str(d) for d in ok)})")
    keep = model.compute_dtype
    model.compute_dtype = dtype
    return keep


def needs_lift(w: torch.Tensor) -> bool:
    return w.dim() == 4 or (w.dim() == 5 and w.shape[2] == 1 and w.shape[-1] == 3)


def lift_params(P: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Parameters in the shapes the 3-D kernels take.  Conv2d (Cout,Cin,3,3) and anisotropic Conv3d (Cout,Cin,1,3,3) weights
    become (Cout,Cin,3,3,3) with only the centre z-tap non-zero; other 4-D weights (1x1 convs, ConvTranspose2d (Cin,Cout,2,2))
    get a unit z extent (a view).  Everything else passes through."""
    Q = {}
    for k, w in P.items():
        if w.dim() == 4 and w.shape[-1] == 3:
            w5 = torch.zeros(w.shape[:2] + (3, 3, 3), dtype=torch.float32, device=w.device)
            w5[:, :, 1] = w
            Q[k] = w5
        elif w.dim() == 5 and w.shape[2] == 1 and w.shape[-1] == 3:
            w5 = torch.zeros(w.shape[:2] + (3, 3, 3), dtype=torch.float32, device=w.device)
            w5[:, :, 1] = w[:, :, 0]
            Q[k] = w5
        elif w.dim() == 4:
            Q[k] = w.reshape(w.shape[:2] + (1,) + w.shape[2:])
        else:
            Q[k] = w
    return Q


def unlift_grads(G: Dict[str, torch.Tensor], P: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Gradients of lifted parameters back in the shapes of the module's parameters (centre z-tap / dropped unit extent)."""
    out = {}
    for n, p in P.items():
        if n not in G:
            continue
        g = G[n]
        if g.shape != p.shape:
            g = g[:, :, 1].reshape(p.shape) if p.shape[-1] == 3 else g.reshape(p.shape)
        out[n] = g if g.is_contiguous() else g.contiguous()
    return out


def channel_pad_plan(cfg: "NetConfig") -> Optional[Dict[str, Tuple]]:
    """For a configuration whose widths were rounded up to multiples of 16: parameter name -> (segments of dim 0, segments of dim 1), a segment =
    (true channels, padded channels); dim 1 is None for vectors.  The decoder blocks' input is the concatenation [up-sampled | skip]: two segments."""
    if cfg.true_feature_maps is None:
        return None
    ft, fp, Lv = list(cfg.true_feature_maps), list(cfg.feature_maps), cfg.depth
    seg = lambda i: (ft[i], fp[i])                                         # noqa: E731
    plan: Dict[str, Tuple] = {}

    def block(prefix, first, cin, cout):
        k = block_keys(prefix, first)
        plan[k["w1"]], plan[k["wsc"]] = ([cout], cin), ([cout], cin)
        plan[k["w2"]] = ([cout], [cout])
        for n in ("b1", "g1", "be1", "b2", "bsc"):
            plan[k[n]] = ([cout], None)
        if not first:
            plan[k["g0"]], plan[k["be0"]] = (cin, None), (cin, None)

    for i in range(Lv):
        block(f"down_path.{i}", i == 0, [(cfg.in_ch, cfg.in_ch)] if i == 0 else [seg(i - 1)], seg(i))
    block("bottleneck", False, [seg(Lv - 1)], seg(Lv))
    for j, i in enumerate(range(Lv - 1, -1, -1)):
        plan[f"up_paths.0.{j}.up.weight"] = ([seg(i + 1)], [seg(i + 1)])   # ConvTranspose: (Cin, Cout, ...)
        plan[f"up_paths.0.{j}.up.bias"] = ([seg(i + 1)], None)
        block(f"up_paths.0.{j}.conv_block", False, [seg(i + 1), seg(i)], seg(i))
    for h in range(len(cfg.out_channels)):
        plan[f"heads.{h}.weight"] = (None, [seg(0)])
    return plan


def _pad_dim(t: torch.Tensor, dim: int, segs) -> torch.Tensor:
    if segs is None or all(a == b for a, b in segs):
        return t
    parts, o = [], 0
    for a, b in segs:
        parts.append(t.narrow(dim, o, a))
        o += a
        if b > a:
            shape = list(t.shape)
            shape[dim] = b - a
            parts.append(t.new_zeros(shape))
    return torch.cat(parts, dim)


def _unpad_dim(t: torch.Tensor, dim: int, segs) -> torch.Tensor:
    if segs is None or all(a == b for a, b in segs):
        return t
    parts, o = [], 0
    for a, b in segs:
        parts.append(t.narrow(dim, o, a))
        o += b
    return torch.cat(parts, dim) if len(parts) > 1 else parts[0]


def pad_channels(P: Dict[str, torch.Tensor], plan) -> Dict[str, torch.Tensor]:
    """Parameters with their channel dimensions zero-padded to the kernels' widths (channel_pad_plan)."""
    Q = {}
    for k, w in P.items():
        s0, s1 = plan.get(k, (None, None))
        Q[k] = _pad_dim(_pad_dim(w, 0, s0), 1, s1).contiguous()
    return Q


def unpad_channel_grads(G: Dict[str, torch.Tensor], plan) -> Dict[str, torch.Tensor]:
    """The parameters' own entries of the padded gradients (the padded rows / columns hold gradients of weights that do not exist)."""
    out = {}
    for k, g in G.items():
        s0, s1 = plan.get(k, (None, None))
        out[k] = _unpad_dim(_unpad_dim(g, 0, s0), 1, s1)
    return out


def input_pad_keys(P: Dict[str, torch.Tensor]) -> List[str]:
    """The parameters whose dim 1 is the image's channels: the first block's 3x3x3 weight and, in the residual network, its shortcut."""
    k = block_keys("down_path.0", True)
    return [n for n in (k["w1"], k["wsc"]) if n in P]


def pad_input_channels(P: Dict[str, torch.Tensor], cin: int) -> Dict[str, torch.Tensor]:
    """Parameters with the input-channel dimension of the first block's weights zero-padded to ``cin`` (NetConfig.true_in_ch -> in_ch); every
    other entry is the caller's own tensor.  The padded weights are views of one zero-filled scratch: one fill and one copy per weight."""
    Q = dict(P)
    keys = input_pad_keys(P)
    shapes = [(P[n].shape[0], cin) + tuple(P[n].shape[2:]) for n in keys]
    offs, tot = [], 0
    for sh in shapes:
        offs.append(tot)
        tot += (math.prod(sh) + 63) // 64 * 64            # keep every weight 256-byte aligned
    flat = P[keys[0]].new_zeros(tot)
    for n, sh, o in zip(keys, shapes, offs):
        Q[n] = flat[o:o + math.prod(sh)].view(sh)
        Q[n][:, :P[n].shape[1]].copy_(P[n])
    return Q


def unpad_input_grads(G: Dict[str, torch.Tensor], c: int) -> Dict[str, torch.Tensor]:
    """The first ``c`` input-channel columns of the padded gradients (the others belong to weights that do not exist)."""
    out = dict(G)
    for n in input_pad_keys(G):
        out[n] = G[n][:, :c].contiguous()
    return out


def block_keys(prefix: str, first: bool) -> Dict[str, str]:
    """Reference state_dict keys of one ResConvBlock."""
    i = 0 if first else 2
    k = {
        "w1": f"{prefix}.block.{i}.block.0.weight", "b1": f"{prefix}.block.{i}.block.0.bias",
        "g1": f"{prefix}.block.{i}.block.1.weight", "be1": f"{prefix}.block.{i}.block.1.bias",
        "w2": f"{prefix}.block.{i + 1}.block.0.weight", "b2": f"{prefix}.block.{i + 1}.block.0.bias",
        "wsc": f"{prefix}.shortcut.0.weight", "bsc": f"{prefix}.shortcut.0.bias",
    }
    if not first:
        k["g0"] = f"{prefix}.block.0.weight"
        k["be0"] = f"{prefix}.block.0.bias"
    return k


class _Stats:
    """Partial-statistics scratch (its finalize into norm records: ResUNetEngine._norm_finalize, _norm_records, _cat_records)."""

    @staticmethod
    def alloc(B, tiles, C, dev):
        return torch.empty((B, tiles, 2, C), dtype=torch.float32, device=dev)

    @staticmethod
    def finalize_cat(parts, B, count, gamma, beta, rec, groups, st):
        """GroupNorm(groups) records of torch.cat(producers, 1): parts = [(partials, tiles, C), ...] in channel order.  A group may straddle
        the boundary between two producers (8 groups over 48 channels = 6 per group), so the per-channel totals of all of them are
        gathered first (bpx_norm_channel_sums) and one more kernel forms the group statistics (bpx_groupnorm_finalize)."""
        Ct = sum(c for _, _, c in parts)
        sums = torch.empty((B, Ct, 2), dtype=torch.float64, device=rec.device)
        off = 0
        for part, tiles, c in parts:
            L.check(lib.bpx_norm_channel_sums(part.data_ptr(), B, tiles, c, sums.data_ptr(), Ct, off, st))
            off += c
        L.check(lib.bpx_groupnorm_finalize(sums.data_ptr(), B, Ct, count, gamma.data_ptr(), beta.data_ptr(), EPS, groups, rec.data_ptr(), st))


_BN_BUFFERS = (".running_mean", ".running_var", ".num_batches_tracked")


def bn_layers(cfg: "NetConfig") -> List[str]:
    """Module names of every norm layer of the network (forward order); their parameters / buffers are ``name + ".weight"`` etc."""
    prefixes = [(f"down_path.{i}", i == 0) for i in range(cfg.depth)] + [("bottleneck", False)]
    prefixes += [(f"up_paths.0.{j}.conv_block", False) for j in range(cfg.depth)]
    out = []
    for prefix, first in prefixes:
        k = block_keys(prefix, first)
        out += ([] if first else [k["g0"][:-len(".weight")]]) + [k["g1"][:-len(".weight")]]
    return out


def _recs(B, C, dev):
    return torch.empty((B, C, 4), dtype=torch.float32, device=dev)


@dataclass
class _Blk:
    """Everything the backward needs about one residual block."""
    keys: Dict[str, str]
    first: bool
    S: Tuple[int, int, int]
    cin: int
    cout: int
    x: Optional[torch.Tensor] = None      # raw block input buffer (NDHWC) - None for the first block (image)
    x_c0: int = 0                          # channel offset / count of the input view inside x
    rec_x: Optional[torch.Tensor] = None
    h: Optional[torch.Tensor] = None
    rec_h: Optional[torch.Tensor] = None
    out: Optional[torch.Tensor] = None     # buffer holding the block output
    out_c0: int = 0
    drop_p: float = 0.0                    # dropout of the block (blocks.py:163), active in training mode only
    site: int = 0                          # index of the block's dropout site (its own random stream)
    a: Optional[torch.Tensor] = None       # with dropout: the materialised act(norm(h)) * keep / (1 - p) the second convolution read
    drop_ctr: Optional[torch.Tensor] = None  # with dropout: the device step counter value THIS forward drew its masks with (its backward regenerates them from it)


# ---- batches whose operands pass the kernels' 32-bit span ------------------------------------------------------------------------------
# The kernels address a whole-batch operand with 32-bit offsets inside one 2 GiB buffer window.  A batch whose largest operand reaches that
# span runs as consecutive sample groups, each under it: the forward of every group, then the backward of every group, with the weight
# gradients of the groups summed in group order (two identical calls give identical bits).  Below the span a batch runs as one group, on
# exactly the launches it always ran.  Training in the 16-bit modes bounds the operands' bytes (the 2 GiB buffer windows of the bf16 / mixed
# backward kernels); inference, and fp32 training, whose kernels address with 64-bit pointers and bound element counts, bound elements (the 32-bit
# indices of the elementwise and pointwise passes and of the chunk strides).
SPAN_LIMIT = 1 << 31
SPAN_MARGIN = 1 << 20      # pitch rounding of the chunk-planar buffers (their plane padding, L.PLANE_PAD_BYTES, is added to it)


def span_in_bytes(dtype: torch.dtype, training: bool) -> bool:
    """Whether batch_groups bounds bytes (16-bit training) or elements (inference, fp32 training)."""
    return training and dtype != torch.float32


def sample_span(cfg: NetConfig, dtype: torch.dtype, patch: Sequence[int], training: bool, unet: bool = False) -> Tuple[int, str]:
    """(span of the largest operand of ONE sample of a (Z, Y, X) patch, what it is): bytes or elements as span_in_bytes says.  ``unet``: the
    U-Net engine's decoder inputs ([up (fm[i]) | skip (fm[i])]) instead of the ResUNet's ([up (fm[i + 1]) | skip (fm[i])])."""
    es = 4 if dtype == torch.float32 else 2
    fm = list(cfg.feature_maps)
    Lv = cfg.depth
    S = [tuple(int(v) for v in patch)]
    for i in range(Lv):
        S.append((max(1, S[i][0] // cfg.z_down[i]), S[i][1] // 2, S[i][2] // 2))
    vox = [s[0] * s[1] * s[2] for s in S]
    ops = [(vox[0] * cfg.in_ch, 4, f"input ({cfg.in_ch} channels)")]
    for i in range(Lv):
        ops.append((vox[i] * fm[i], es, f"level-{i} activation ({fm[i]} channels)"))
        cc = 2 * fm[i] if unet else fm[i] + fm[i + 1]
        ops.append((vox[i] * cc, es, f"level-{i} decoder input ({cc} channels)"))
    ops.append((vox[Lv] * fm[Lv], es, f"bottleneck activation ({fm[Lv]} channels)"))
    vo = vox[0] * (cfg.post_up * 4 if cfg.post_up else 1)
    if cfg.post_up:
        ops.append((vo * fm[0], es, f"up-sampled level-0 activation ({fm[0]} channels)"))
    ops.append((vo * sum(cfg.out_channels), 4, f"logits ({sum(cfg.out_channels)} channels)"))
    nb = span_in_bytes(dtype, training)
    n, _, what = max((e * (b if nb else 1), -k, w) for k, (e, b, w) in enumerate(ops))
    return n, what


def _plane_pad(cfg: NetConfig, unet: bool) -> int:
    """Bytes a chunk-planar decoder input adds for its plane padding (L.PLANE_PAD_BYTES between consecutive 16-channel planes)."""
    fm = list(cfg.feature_maps)
    widest = max((2 * fm[i] if unet else fm[i] + fm[i + 1]) for i in range(cfg.depth))
    return L.PLANE_PAD_BYTES * (widest // 16)


def batch_groups(cfg: NetConfig, dtype: torch.dtype, B: int, patch: Sequence[int], training: bool, unet: bool = False) -> List[Tuple[int, int]]:
    """Sample ranges [a, b) a batch of B patches runs as: [(0, B)] while its largest operand stays under the span, otherwise the fewest
    groups of near-equal size (larger ones first) that each stay under it.  Raises NotImplementedError when one sample alone is beyond
    it (on the host, before anything is launched)."""
    per, what = sample_span(cfg, dtype, patch, training, unet)
    unit = "bytes" if span_in_bytes(dtype, training) else "elements"
    margin = SPAN_MARGIN + _plane_pad(cfg, unet)
    if per + margin > SPAN_LIMIT:
        raise NotImplementedError(f"patch {'x'.join(str(int(v)) for v in patch)}: one sample's {what} spans {per} {unit}, beyond the per-sample limit "
                                  f"of 2^31 {unit} ({SPAN_LIMIT - margin} with the buffers' padding) of the MI355X kernels' 32-bit addressing")
    if B * per + margin <= SPAN_LIMIT:
        return [(0, B)]
    g = (SPAN_LIMIT - margin) // per
    n = -(-B // g)
    out, a = [], 0
    for q in range(n):
        b = a + B // n + (1 if q < B % n else 0)
        out.append((a, b))
        a = b
    return out


class ResUNetEngine:
    _unet_layout = False          # batch_groups: the U-Net engine's decoder inputs are [up (fm[i]) | skip (fm[i])]

    def __init__(self, cfg: NetConfig, dtype: torch.dtype = torch.bfloat16):
        assert dtype in (torch.bfloat16, torch.float32, torch.float16)
        self.cfg = cfg
        self.dtype = dtype
        self._pad_plan = channel_pad_plan(cfg) if type(self) is ResUNetEngine else None      # zero-padded widths: this engine's own forward / backward only
        if cfg.true_feature_maps is not None and type(self) is not ResUNetEngine:
            raise NotImplementedError(f"feature_maps {list(cfg.true_feature_maps)} (not multiples of 16): only the ResUNet engine pads them")
        if type(self) is not ResUNetEngine and list(cfg.feature_maps)[0] not in (16, 32):
            raise NotImplementedError("output head supports 16 or 32 features (the GEMM-fed head for wider first levels is the ResUNet engine's)")
        # float16 = the same 16 bits per element with an 11-bit mantissa: the mode whose forward agrees with the fp32 reference to Dice
        # delta < 1e-4 at the speed of the bf16 mode.  Its TRAINING form is mixed (BPX_MIX16): the forward pass and every stored
        # activation are fp16, every gradient tensor and the backward MFMA operands are bf16 (fp32 exponent range: no loss scaling) -
        # the backward kernels read the fp16 activations and convert on the way to their bf16 operands.
        self.dt = {torch.bfloat16: L.BF16, torch.float32: L.F32, torch.float16: L.F16}[dtype]
        mixed = dtype == torch.float16
        self.gdtype = torch.bfloat16 if mixed else dtype         # storage type of gradient tensors
        self.gdt = L.BF16 if mixed else self.dt                  # dtype code of kernels that touch gradient tensors only
        self.bdt = L.MIX16 if mixed else self.dt                 # dtype code of backward kernels that also read a forward activation
        self.pdt = L.MIX16 if mixed else self.dt                 # weight packing: forward operators in the forward type, transposed ones in bf16
        self.act = L.ACT[cfg.activation]
        self._ws: Optional[torch.Tensor] = None
        self._keep: Optional[List[torch.Tensor]] = None      # per backward pass (_backward_pass)
        self._deferred = False
        # dropout (p > 0 levels, training mode): see _drop_args
        self.drop_active = False               # set by the module before every forward (= module.training)
        self.drop_seed: Optional[int] = None
        self._drop_counter: Optional[torch.Tensor] = None
        self.drop_mask_io: Optional[Dict[int, torch.Tensor]] = None   # tests: {site: uint8 keep flags}; drop_mask_mode 1 = use them, 2 = record the drawn ones
        self.drop_mask_mode = 0
        self._pack_cache: Dict[Tuple[int, int, int], torch.Tensor] = {}
        self._pack_versions: Dict[Tuple[int, int, int], Tuple[int, int]] = {}
        # BatchNorm ('bn'): batch statistics and running-buffer updates (training) or records from the running buffers (eval); the module sets
        # bn_training (= module.training) and bn_hparams {layer name: (eps, momentum)} before every forward; without them: (1e-5, 0.1)
        self.bn = cfg.normalization == "bn"
        self.bn_training = True
        self.bn_hparams: Dict[str, Tuple[float, Optional[float]]] = {}
        self._bn_steps = 0                      # training-mode forwards: the kernels update the running buffers without a version bump
        self._bn_cache = None
        self._bn_eval: Optional[Dict[str, torch.Tensor]] = None      # eval-mode records of the running forward
        self._bn_running = 0                                          # the backward's forward ran in eval mode (bpx_batchnorm_bwd_finalize)

    def clear_caches(self) -> None:
        """Drop the packed / lifted weight copies and BatchNorm eval records kept for inference (ResUNet.train() calls this)."""
        self._pack_cache.clear()
        self._pack_versions.clear()
        self._lift_cache = None
        self._bn_cache = None

    # ---- BatchNorm ------------------------------------------------------------------------------------
    def _bn_hp(self, layer: str) -> Tuple[float, float]:
        eps, mom = self.bn_hparams.get(layer, (EPS, 0.1))
        if mom is None:
            raise NotImplementedError(f"normalization='bn': {layer} has momentum=None (cumulative moving average); the MI355X engine implements a float momentum")
        return float(eps), float(mom)

    def _norm_finalize(self, P, layer: str, part, B, tiles, C, count, rec, rec_ld, rec_off, st, lo: int = 0):
        """Records of channels [lo, lo + C) of norm layer `layer` from one producer's partials (training mode; eval-mode BN records come from
        _bn_eval_records).  BatchNorm updates the running buffers of those channels; num_batches_tracked with the call that covers channel 0."""
        g, b = P[layer + ".weight"], P[layer + ".bias"]
        if not self.bn:      # InstanceNorm (one group per channel) or GroupNorm(gn_groups) records of ONE producer's tensor
            L.check(lib.bpx_norm_finalize(part.data_ptr(), B, tiles, C, count, g[lo:].data_ptr(), b[lo:].data_ptr(), EPS, self.cfg.gn_groups or C,
                                          rec.data_ptr(), rec_ld, rec_off, st))
            return
        eps, mom = self._bn_hp(layer)
        rm, rv, nbt = (P.get(layer + s) for s in _BN_BUFFERS)
        L.check(lib.bpx_batchnorm_finalize(part.data_ptr(), B, tiles, C, count, g[lo:].data_ptr(), b[lo:].data_ptr(), eps, mom,
                                           None if rm is None else rm[lo:].data_ptr(), None if rv is None else rv[lo:].data_ptr(),
                                           L.ptr(nbt) if lo == 0 else None, rec.data_ptr(), rec_ld, rec_off, st))

    def _norm_records(self, P, layer: str, part, tiles, C, vox, st) -> torch.Tensor:
        """The (B, C, 4) records of norm layer `layer` on ONE producer's tensor: the running-buffer records of an eval-mode BatchNorm forward,
        else new ones from the producer's partials (B, tiles, 2, C)."""
        if self._bn_eval is not None:
            return self._bn_eval[layer]
        B = part.shape[0]
        rec = _recs(B, C, part.device)
        self._norm_finalize(P, layer, part, B, tiles, C, vox, rec, C, 0, st)
        return rec

    def _cat_records(self, P, layer: str, parts, B, vox, dev, st) -> torch.Tensor:
        """The records of norm layer `layer` on torch.cat(producers, 1): parts = [(partials, tiles, C), ...] in channel order.  A GroupNorm group may
        straddle two producers (_Stats.finalize_cat); InstanceNorm and BatchNorm finalize each producer's column range (of the records, of gamma /
        beta and of the running buffers) on its own."""
        if self._bn_eval is not None:
            return self._bn_eval[layer]
        Ct = sum(c for _, _, c in parts)
        rec = _recs(B, Ct, dev)
        if self.cfg.gn_groups:
            _Stats.finalize_cat(parts, B, vox, P[layer + ".weight"], P[layer + ".bias"], rec, self.cfg.gn_groups, st)
            return rec
        lo = 0
        for part, tiles, c in parts:
            self._norm_finalize(P, layer, part, B, tiles, c, vox, rec, Ct, lo, st, lo=lo)
            lo += c
        return rec

    def _bn_eval_records(self, P, B, dev, cache: bool) -> Dict[str, torch.Tensor]:
        """{layer: (B, C, 4) records} of every BN layer from the running buffers, ONE launch (bpx_batchnorm_eval_records).  Kept while the
        parameters and buffers keep their storage and version, weights_epoch() and the count of training-mode forwards (load_state_dict copies in
        place: a new version) and the layers' eps; a captured forward computes them inside the graph (cache = False), so a replay reads the buffers
        of its time."""
        layers = bn_layers(self.cfg)
        ts = [P[n + s] for n in layers for s in (".weight", ".bias", ".running_mean", ".running_var")]
        eps = [float(self.bn_hparams.get(n, (EPS, None))[0]) for n in layers]
        key = (B, dev, _WEIGHTS_EPOCH[0], self._bn_steps, tuple(eps)) + tuple((t.data_ptr(), t._version) for t in ts)
        if cache and self._bn_cache is not None and self._bn_cache[0] == key:
            return self._bn_cache[1]
        if any(t.dtype != torch.float32 or not t.is_contiguous() for t in ts):
            raise TypeError("normalization='bn': weight, bias, running_mean and running_var must be contiguous float32 tensors")
        Cs = [P[n + ".weight"].numel() for n in layers]
        buf = torch.empty((B * sum(Cs), 4), dtype=torch.float32, device=dev)
        jobs = (L.BnEvalJob * len(layers))()
        recs, o = {}, 0
        for q, (n, c) in enumerate(zip(layers, Cs)):
            recs[n] = buf[o:o + B * c].view(B, c, 4)
            jobs[q] = L.BnEvalJob(P[n + ".weight"].data_ptr(), P[n + ".bias"].data_ptr(), P[n + ".running_mean"].data_ptr(),
                                  P[n + ".running_var"].data_ptr(), recs[n].data_ptr(), c, eps[q])
            o += B * c
        L.check(lib.bpx_batchnorm_eval_records(len(layers), C.cast(jobs, C.c_void_p), B, L.stream_ptr()))
        self._bn_cache = (key, recs) if cache else None
        return recs

    # ---- one backward pass -----------------------------------------------------------------------------
    @contextlib.contextmanager
    def _backward_pass(self, defer: bool):
        """The state of one backward pass: ``self._keep``, the buffers its queued kernels still read, and with ``defer`` the deferred
        weight-gradient window (bpx_wgrad_defer_begin): the step's reductions run as one batched launch at the flush.  The flush runs on
        every exit, an exception included, and neither the window nor the list outlives the pass."""
        self._keep, self._deferred = [], defer
        if defer:
            L.check(lib.bpx_wgrad_defer_begin())
        try:
            yield
        finally:
            try:
                if defer:
                    L.check(lib.bpx_wgrad_defer_flush(L.stream_ptr()))
            finally:
                self._keep, self._deferred = None, False

    def _workspace(self, nbytes: int, dev) -> torch.Tensor:
        """Scratch for the wgrad partial sums.  Deferred reductions (backward): one slab per call, kept until the flush.
        Otherwise grow-only (launches are stream-ordered, so one slab is enough)."""
        if self._deferred:
            ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
            self._keep.append(ws)
            return ws
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(max(nbytes, 32 << 20), dtype=torch.uint8, device=dev)
        return self._ws

    def _grad_slab(self, P: Dict[str, torch.Tensor], dev) -> Dict[str, torch.Tensor]:
        """Parameter gradients as views of ONE zero-filled fp32 slab in parameter order (the wgrad kernels accumulate into them);
        the slab is ``self.last_flat_grad``.  BatchNorm running buffers have no gradient."""
        names = [n for n in P if not n.endswith(_BN_BUFFERS)]
        flat = torch.zeros(sum(P[n].numel() for n in names), dtype=torch.float32, device=dev)
        self.last_flat_grad = flat
        G, o = {}, 0
        for n in names:
            G[n] = flat[o:o + P[n].numel()].view(P[n].shape)
            o += P[n].numel()
        return G

    # ---- sample groups (batch_groups) -------------------------------------------------------------------
    def _groups_for(self, B: int, patch, save: bool) -> List[Tuple[int, int]]:
        """The sample groups of a forward; BatchNorm couples the samples of a batch and keeps running it as one group."""
        groups = [(0, B)] if self.bn else batch_groups(self.cfg, self.dtype, B, patch, save, unet=self._unet_layout)
        self.last_groups = groups
        return groups

    def _forward_groups(self, groups, fwd, x: torch.Tensor, save: bool, x_ndhwc: Optional[torch.Tensor] = None, **kw):
        """The forward of every group in turn; logits concatenated along the batch."""
        outs, parts = [], []
        for a, b in groups:
            if x_ndhwc is not None:
                lo, c = fwd(x=None, x_ndhwc=x_ndhwc[a:b], save=save, **kw)
            else:
                lo, c = fwd(x=x[a:b], save=save, **kw)
            outs.append(lo)
            parts.append(((a, b), c))
        self.last_groups = list(groups)
        return torch.cat(outs, 0), (dict(groups=parts) if save else None)

    def _backward_groups(self, ctx, dlogits: torch.Tensor, bwd, on_last_block=None) -> Dict[str, torch.Tensor]:
        """The backward of every group in turn (with the packed operands of its own forward); the groups' parameter gradients are summed in
        group order, the input gradient ("__dx__") is concatenated."""
        G, flat, dx = None, None, []
        for (a, b), c in ctx["groups"]:
            Gi = bwd(c, dlogits[a:b])
            if "__dx__" in Gi:
                dx.append(Gi.pop("__dx__"))
            if G is None:
                G, flat = Gi, getattr(self, "last_flat_grad", None)
            else:
                for k, v in Gi.items():
                    G[k].add_(v)
        if flat is not None:
            self.last_flat_grad = flat
        if dx:
            G["__dx__"] = torch.cat(dx, 0)
        if on_last_block is not None:
            on_last_block()          # every gradient is final here
        return G

    # ---- dropout --------------------------------------------------------------------------------------
    # nn.Dropout(p) of a block sits behind Conv -> Norm -> Act of its first ConvBlock (blocks.py:163), i.e. on the tensor the second convolution's
    # fused prologue would form on the fly.  For p > 0 in training mode that tensor is materialised with the mask applied
    # (bpx_norm_act_dropout_fwd), the second convolution runs without a prologue, and its backward is the plain dgrad followed by
    # bpx_norm_act_dropout_bwd (mask, activation derivative, IN-backward sums).  The mask is a counter-based function of (seed, step counter, site,
    # element): nothing is stored, a replayed graph draws a new mask at every step because the counter lives on the device.
    def _drop_state(self, dev):
        if self.drop_seed is None:
            self.drop_seed = int(torch.initial_seed()) & ((1 << 63) - 1)
        if self._drop_counter is None or self._drop_counter.device != dev:
            self._drop_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        return self._drop_counter

    def _drop_mask(self, blk: "_Blk", numel: int, dev):
        """(pointer, mode) of the test hook's keep-flag buffer for this site."""
        if not self.drop_mask_mode:
            return None, 0
        if self.drop_mask_io is None:
            self.drop_mask_io = {}
        m = self.drop_mask_io.get(blk.site)
        if m is None:
            assert self.drop_mask_mode == 2, f"dropout site {blk.site}: no mask given"
            m = self.drop_mask_io[blk.site] = torch.zeros(numel, dtype=torch.uint8, device=dev)
        assert m.numel() == numel and m.dtype == torch.uint8 and m.is_cuda
        return m.data_ptr(), self.drop_mask_mode

    def _wgrad(self, B, S, x: "L.Tensor", rec, act, dy: "L.Tensor", k, dw, db, st, dev, db2=None):
        """db2: a second bias gradient that takes the same sums (the shortcut bias of a residual block)."""
        D, H, W = S
        nb = lib.bpx_conv3d_wgrad_workspace(B, D, H, W, x.C, dy.C, k)
        ws = self._workspace(nb, dev)
        L.check(lib.bpx_conv3d_wgrad_db2(self.bdt, B, D, H, W, x, L.ptr(rec), act, dy, k, dw.data_ptr(), L.ptr(db), L.ptr(db2), ws.data_ptr(), ws.numel(), st))

    def _bwd_fused_ok(self, B, S, Ct: int, Cdy: int, act: Optional[int] = None) -> bool:
        """One-pass dgrad + wgrad (bpx_conv3d_bwd_fused) for this conv, whose prologue applies `act` (default: the network's)?"""
        act = self.act if act is None else act
        return (act <= 3 and self.cfg.gn_groups == 0 and self.dtype != torch.float32
                and bool(lib.bpx_conv3d_bwd_fused_supported(self.bdt, B, S[0], S[1], S[2], Ct, Cdy)))

    def _dgrad_prologue(self, B, S, dy: "L.Tensor", wt, t: "L.Tensor", rec, act, g: "L.Tensor", st, *, fused: bool, dw=None, db=None, db2=None):
        """Input gradient of ``conv3(act(norm(t)))`` into g, times act', with the norm backward's reduction partials -> (tiles, red).  ``fused``
        (the caller asked _bwd_fused_ok): one pass over (dy, t) that also forms the conv's weight / bias gradients dw, db (db2: a second bias that
        takes the same sums); otherwise the dgrad kernel alone - the caller issued the conv's _wgrad."""
        D, H, W = S
        dev = rec.device
        if fused:
            tiles = lib.bpx_conv3d_bwd_fused_stats_tiles(B, D, H, W, t.C, dy.C)
            red = torch.empty((B, tiles, 2, t.C), dtype=torch.float32, device=dev)
            ws = self._workspace(lib.bpx_conv3d_bwd_fused_workspace(B, D, H, W, t.C, dy.C), dev)
            L.check(lib.bpx_conv3d_bwd_fused(self.bdt, B, D, H, W, dy, wt.data_ptr(), t, rec.data_ptr(), act, g, red.data_ptr(),
                                             dw.data_ptr(), L.ptr(db), L.ptr(db2), ws.data_ptr(), ws.numel(), st))
        else:
            tiles = lib.bpx_conv3d_stats_tiles(self.dt, B, D, H, W, t.C)
            red = torch.empty((B, tiles, 2, t.C), dtype=torch.float32, device=dev)
            L.check(lib.bpx_conv3d_dgrad(self.bdt, B, D, H, W, dy, wt.data_ptr(), t, rec.data_ptr(), act, g, red.data_ptr(), st))
        return tiles, red

    def _norm_bwd_coef(self, red, B, tiles, C, vox, rec, gamma, dgamma, dbeta, st, *, deferred: bool) -> torch.Tensor:
        """Norm backward finalize: the reduction partials `red` (B, tiles, 2, C) of a dgrad prologue or of bpx_norm_act_bwd -> the (B, C, 4)
        coefficients bpx_norm_bwd_apply and the pointwise hand-over kernels read; dgamma / dbeta (either may be None) take the affine gradients.
        ``deferred``: dgamma / dbeta arrive with the flush of the pass's weight-gradient reductions, `red` holds their per-sample terms until then."""
        coef = torch.empty((B, C, 4), dtype=torch.float32, device=red.device)
        gng = self.cfg.gn_groups
        if self.bn:
            L.check(lib.bpx_batchnorm_bwd_finalize(red.data_ptr(), B, tiles, C, vox, rec.data_ptr(), gamma.data_ptr(), L.ptr(dgamma), L.ptr(dbeta),
                                                   self._bn_running, coef.data_ptr(), st))
        elif gng and (C // gng) not in (1, 2, 4, 8, 16, 32, 64):
            # the concatenated decoder input: 6 / 12 / 24 / 48 channels per group -> per-channel totals, then the general group kernel.  Never a
            # block's own width: NetConfig.__post_init__ rejects GroupNorm widths outside the power-of-two set
            sums = torch.empty((B, C, 2), dtype=torch.float64, device=red.device)
            L.check(lib.bpx_norm_channel_sums(red.data_ptr(), B, tiles, C, sums.data_ptr(), C, 0, st))
            L.check(lib.bpx_groupnorm_bwd_finalize(sums.data_ptr(), B, C, vox, rec.data_ptr(), gamma.data_ptr(), L.ptr(dgamma), L.ptr(dbeta), gng,
                                                   coef.data_ptr(), st))
        elif deferred:
            self._keep.append(red)
            L.check(lib.bpx_norm_bwd_finalize_deferred(red.data_ptr(), B, tiles, C, vox, rec.data_ptr(), gamma.data_ptr(), L.ptr(dgamma), L.ptr(dbeta),
                                                       gng or C, coef.data_ptr(), st))
        else:
            L.check(lib.bpx_norm_bwd_finalize(red.data_ptr(), B, tiles, C, vox, rec.data_ptr(), gamma.data_ptr(), L.ptr(dgamma), L.ptr(dbeta), gng or C,
                                              coef.data_ptr(), st))
        return coef

    def _norm_act_bwd(self, raw: torch.Tensor, rec, act, dA: "L.Tensor", gamma, dgamma, dbeta, st) -> torch.Tensor:
        """Backward of a materialised ``act(IN(raw))`` (raw: a dense NDHWC tensor): dA -> d(raw), a new gradient tensor.  The elementwise
        product with act' and the two InstanceNorm reductions, finalize, apply.  (Mixed mode: raw is the forward's fp16 tensor, d(raw) bf16.)"""
        B, C, dev = raw.shape[0], raw.shape[-1], raw.device
        vox = raw.numel() // (B * C)
        tiles = lib.bpx_norm_act_tiles(self.gdt, vox, C)
        red = torch.empty((B, tiles, 2, C), dtype=torch.float32, device=dev)
        g = torch.empty(raw.shape, dtype=self.gdtype, device=dev)
        L.check(lib.bpx_norm_act_bwd(self.bdt, B, vox, dA, L.tview(raw), rec.data_ptr(), act, L.NULL_T, L.tview(g), red.data_ptr(), st))
        coef = self._norm_bwd_coef(red, B, tiles, C, vox, rec, gamma, dgamma, dbeta, st, deferred=False)
        L.check(lib.bpx_norm_bwd_apply(self.bdt, B, vox, L.tview(g), L.tview(raw), coef.data_ptr(), L.NULL_T, L.tview(g), st))
        return g

    def _convT_bwd(self, P, G, B, Sl, sz, x_in: torch.Tensor, dUp: torch.Tensor, wk: str, bk: str, Cin: int, Cout: int, st, dev) -> torch.Tensor:
        """Backward of ConvTranspose3d(Cin, Cout, k = s = (sz, 2, 2)) on x_in (B, *Sl, Cin): dUp -> the new d(x_in), with the weight / bias gradients
        into G[wk], G[bk] (bpx_convT3d_k2s2_bwd: from ONE pass over dUp at the 32 -> 32 level of a large volume, else the two kernels)."""
        ws = self._workspace(lib.bpx_convT3d_k2s2_wgrad_workspace(B, Sl[0], Sl[1], Sl[2], sz, Cin, Cout), dev)
        dx = torch.empty((B,) + tuple(Sl) + (Cin,), dtype=self.gdtype, device=dev)
        wt = self._pack(P[wk], L.PK_CT_T if sz == 2 else L.PK_CT4_T, Cin, Cout, False)
        L.check(lib.bpx_convT3d_k2s2_bwd(self.bdt, B, Sl[0], Sl[1], Sl[2], sz, L.tview(x_in), L.tview(dUp), wt.data_ptr(), L.tview(dx),
                                         G[wk].data_ptr(), G[bk].data_ptr(), ws.data_ptr(), ws.numel(), st))
        self._keep += [dUp, dx]
        return dx

    # ---- heads ----------------------------------------------------------------------------------------
    def _head_matrix(self, P) -> Tuple[torch.Tensor, torch.Tensor]:
        """The heads as ONE (n_out, fm0) matrix and its bias: a single head reads the parameter itself, several are concatenated by rows."""
        outs, fm0 = self.cfg.out_channels, list(self.cfg.feature_maps)[0]
        if len(outs) == 1:
            hw, hb = P["heads.0.weight"], P["heads.0.bias"]
        else:
            hw = torch.cat([P[f"heads.{h}.weight"].reshape(-1, fm0) for h in range(len(outs))], 0)
            hb = torch.cat([P[f"heads.{h}.bias"] for h in range(len(outs))], 0)
        return hw.reshape(sum(outs), fm0).contiguous(), hb

    def _pick16_fwd(self, B, vox, o16: torch.Tensor, n_out: int, head_act: int, logits: torch.Tensor, st) -> torch.Tensor:
        """The first n_out channels of the zero-padded 16-channel tensor o16, through the output activation, into the planar fp32 logits: the head
        kernel with an identity matrix, which is returned (the backward's operand)."""
        eye = torch.eye(n_out, 16, dtype=torch.float32, device=o16.device).contiguous()
        zb = torch.zeros((n_out,), dtype=torch.float32, device=o16.device)
        L.check(lib.bpx_head_fwd(self.dt, vox, B, L.tview(o16), eye.data_ptr(), zb.data_ptr(), n_out, head_act, logits.data_ptr(), n_out * vox, vox, st))
        return eye

    def _pick16_bwd(self, B, vox, o16: torch.Tensor, eye: torch.Tensor, n_out: int, dl: torch.Tensor, st, dev) -> torch.Tensor:
        """Backward of _pick16_fwd: dl (the fp32 logits' gradient) -> the new d(o16); the identity matrix's own gradients are discarded."""
        do16 = torch.empty(o16.shape, dtype=self.gdtype, device=dev)
        eg, ebg = torch.zeros((n_out, 16), dtype=torch.float32, device=dev), torch.zeros((n_out,), dtype=torch.float32, device=dev)
        hws = self._workspace(lib.bpx_head_bwd_workspace(16, n_out), dev)
        L.check(lib.bpx_head_bwd(self.bdt, vox, B, L.tview(o16), eye.data_ptr(), n_out, dl.data_ptr(), n_out * vox, vox, L.tview(do16), eg.data_ptr(),
                                 ebg.data_ptr(), hws.data_ptr(), hws.numel(), st))
        self._keep += [do16, eg, ebg]
        return do16

    def _head_fwd(self, B, So, feat: torch.Tensor, hw: torch.Tensor, hb: torch.Tensor, head_act: int, st, dev):
        """The heads (_head_matrix) on the dense feature tensor -> (planar fp32 logits (B, n_out, *So), what _head_bwd needs of a wide head or None)."""
        n_out, fm0 = hw.shape
        vox = So[0] * So[1] * So[2]
        logits = torch.empty((B, n_out) + tuple(So), dtype=torch.float32, device=dev)
        if fm0 in (16, 32):
            L.check(lib.bpx_head_fwd(self.dt, vox, B, L.tview(feat), hw.data_ptr(), hb.data_ptr(), n_out, head_act, logits.data_ptr(), n_out * vox, vox, st))
            return logits, None
        # wider first level (e.g. FEATURE_MAPS [48, 64, 80, 96] of the reference's Ovarian-Reserve template): the heads' (n_out, fm0) matrix,
        # zero-padded to 16 rows, runs as a 1x1x1 convolution on the pointwise MFMA kernel; the head kernel then picks the real channels of the
        # 16-channel result and applies the output activation.  The logits pass through the 16-bit storage type once.
        w16 = torch.zeros((16, fm0), dtype=torch.float32, device=dev)
        b16 = torch.zeros((16,), dtype=torch.float32, device=dev)
        w16[:n_out] = hw
        b16[:n_out] = hb
        o16 = torch.empty((B,) + tuple(So) + (16,), dtype=self.dtype, device=dev)
        wp16 = self._pack(w16, L.PK_DENSE, fm0, 16, False)
        L.check(lib.bpx_conv1x1_fwd(self.dt, B, vox, L.tview(feat), wp16.data_ptr(), b16.data_ptr(), L.NULL_T, L.NULL_T, None, L.NULL_T, L.tview(o16), st))
        return logits, dict(o16=o16, w16=w16, eye=self._pick16_fwd(B, vox, o16, n_out, head_act, logits, st))

    def _head_bwd(self, G, B, So, feat: "L.Tensor", hw: torch.Tensor, dl: torch.Tensor, dfeat: "L.Tensor", st, dev, wide=None) -> None:
        """Backward of the heads (the (n_out, fm0) matrix hw on `feat`): the input gradient into dfeat, the weight / bias gradients into G's zeroed
        ``heads.{h}`` entries - in place for one head, else through one matrix split by rows.  fm0 = 16 or 32: bpx_head_bwd; ``wide`` (_head_fwd):
        the pick's backward on the 16-channel tensor, then the 1x1x1 convolution's two gradients."""
        outs = list(self.cfg.out_channels)
        n_out, fm0 = sum(outs), feat.C
        vox = So[0] * So[1] * So[2]
        if wide is not None:
            # k = 1 wgrad (rows 0 .. n_out of the padded matrix are the heads') and the pointwise GEMM with the transposed matrix.  The weight gradient
            # is reduced right away (not with the step's batch): its heads' rows are copied out at once.
            do16 = self._pick16_bwd(B, vox, wide["o16"], wide["eye"], n_out, dl, st, dev)
            dw16 = torch.zeros((16, fm0, 1, 1, 1), dtype=torch.float32, device=dev)
            db16 = torch.zeros((16,), dtype=torch.float32, device=dev)
            self._wgrad(B, So, feat, None, 0, L.tview(do16), 1, dw16, db16, st, dev)
            L.check(lib.bpx_wgrad_defer_flush(L.stream_ptr()))
            L.check(lib.bpx_wgrad_defer_begin())
            self._split_heads(G, dw16.view(16, fm0)[:n_out], db16[:n_out])
            wt16 = self._pack(wide["w16"], L.PK_DENSE_T, fm0, 16, False)
            L.check(lib.bpx_conv1x1_fwd(self.gdt, B, vox, L.tview(do16), wt16.data_ptr(), None, L.NULL_T, L.NULL_T, None, L.NULL_T, dfeat, st))
            self._keep += [dw16, db16]
            return
        one_head = len(outs) == 1
        hwg = G["heads.0.weight"] if one_head else torch.zeros((n_out, fm0), dtype=torch.float32, device=dev)
        hbg = G["heads.0.bias"] if one_head else torch.zeros((n_out,), dtype=torch.float32, device=dev)
        hws = self._workspace(lib.bpx_head_bwd_workspace(fm0, n_out), dev)
        L.check(lib.bpx_head_bwd(self.bdt, vox, B, feat, hw.data_ptr(), n_out, dl.data_ptr(), n_out * vox, vox, dfeat, hwg.data_ptr(), hbg.data_ptr(),
                                 hws.data_ptr(), hws.numel(), st))
        if not one_head:
            self._split_heads(G, hwg, hbg)

    def _split_heads(self, G, hwg: torch.Tensor, hbg: torch.Tensor) -> None:
        o = 0
        for h, oc in enumerate(self.cfg.out_channels):
            G[f"heads.{h}.weight"].copy_(hwg[o:o + oc].view(G[f"heads.{h}.weight"].shape))
            G[f"heads.{h}.bias"].copy_(hbg[o:o + oc])
            o += oc

    # ------------------------------------------------------------------------------------------
    def _pack_plan(self, train: bool):
        """(parameter name, pack mode, Cin, Cout) of every packed operand one step needs (forward; + backward if train)."""
        cfg = self.cfg
        fm, Lv = list(cfg.feature_maps), cfg.depth
        plan = []

        def block(prefix, first, cin, cout):
            k = block_keys(prefix, first)
            if not (first and cfg.in_ch == 1):
                plan.append((k["w1"], L.PK_K3, cin, cout))
                plan.append((k["wsc"], L.PK_K1, cin, cout))
            plan.append((k["w2"], L.PK_K3, cout, cout))
            if train:
                plan.append((k["w2"], L.PK_K3_T, cout, cout))
                if not first:
                    plan.append((k["w1"], L.PK_K3_T, cin, cout))
                    plan.append((k["wsc"], L.PK_DENSE_T, cin, cout))

        for i in range(Lv):
            block(f"down_path.{i}", i == 0, cfg.in_ch if i == 0 else fm[i - 1], fm[i])
        block("bottleneck", False, fm[Lv - 1], fm[Lv])
        for j, i in enumerate(range(Lv - 1, -1, -1)):
            cup = fm[i + 1]
            plan.append((f"up_paths.0.{j}.up.weight", L.PK_CT if cfg.z_down[i] == 2 else L.PK_CT4, cup, cup))
            if train:
                plan.append((f"up_paths.0.{j}.up.weight", L.PK_CT_T if cfg.z_down[i] == 2 else L.PK_CT4_T, cup, cup))
            block(f"up_paths.0.{j}.conv_block", False, cup + fm[i], fm[i])
        return plan

    def _prepack(self, P: Dict[str, torch.Tensor], train: bool, dev, plan=None) -> None:
        """Pack every MFMA weight operand of the step with ONE launch into one buffer (the weights change after every
        optimizer step, so training re-packs ~60 small tensors per step).  plan: the (name, mode, Cin, Cout) list to use instead of
        this engine's own (the ResUNet++ engine records its list on the first step)."""
        self._prepacked = {}
        if plan is None:
            plan = self._pack_plan(train)
        if any(P[name].dtype != torch.float32 or not P[name].is_contiguous() for name, _, _, _ in plan):
            return  # _pack() falls back to per-tensor packing (with the conversion copy)
        sizes = [int(lib.bpx_packed_weight_elems(mode, cin, cout, self.dt)) for _, mode, cin, cout in plan]
        offs, tot = [], 0
        for n in sizes:
            offs.append(tot)
            tot += (n + 127) // 128 * 128          # keep every operand 256-byte aligned
        buf = torch.empty(tot, dtype=self.dtype, device=dev)
        jobs = (L.PackJob * len(plan))()
        es = buf.element_size()
        for q, ((name, mode, cin, cout), off) in enumerate(zip(plan, offs)):
            w = P[name]
            jobs[q] = L.PackJob(w.data_ptr(), buf.data_ptr() + off * es, mode, cin, cout, 0)
            self._prepacked[(w.data_ptr(), mode)] = buf[off:off + sizes[q]]
        L.check(lib.bpx_pack_weights_batched(self.pdt, len(plan), C.cast(jobs, C.c_void_p), L.stream_ptr()))

    def _begin_recorded_packs(self, P: Dict[str, torch.Tensor], train: bool, dev, cache_weights: bool) -> None:
        """For the tape engines (ResUNet++, RCAN), whose list of packed operands is not written down: the first step of a kind
        (inference / training) packs its weights one by one and ``_pack`` records which PARAMETERS were packed how; every later step
        packs that list with one launch up front (78 launches -> 1 per ResUNet++ training step, ~820 -> 1 for the RCAN trunk)."""
        if not hasattr(self, "_pack_plans"):
            self._pack_plans = {}
        self._pack_names = {v.data_ptr(): k for k, v in P.items()}
        self._pack_seen = self._pack_plans.setdefault(bool(train), {})
        self._prepacked = {}
        if self._pack_seen and not cache_weights:
            self._prepack(P, train, dev, plan=list(self._pack_seen))

    def _pack(self, w: torch.Tensor, mode: int, cin: int, cout: int, cache: bool) -> torch.Tensor:
        pre = getattr(self, "_prepacked", None)
        if pre:
            hit = pre.get((w.data_ptr(), mode))
            if hit is not None:
                return hit
        names = getattr(self, "_pack_names", None)
        if names:
            name = names.get(w.data_ptr())
            if name is not None:
                self._pack_seen[(name, mode, cin, cout)] = True       # a parameter (not a per-step temporary): part of the next step's batch
        key = (w.data_ptr(), mode, self.dt)
        stamp = (w._version, _WEIGHTS_EPOCH[0])
        if cache and key in self._pack_cache and self._pack_versions.get(key) == stamp:
            return self._pack_cache[key]
        n = lib.bpx_packed_weight_elems(mode, cin, cout, self.dt)
        out = torch.empty(n, dtype=self.dtype, device=w.device)
        wc = w.detach()
        if wc.dtype != torch.float32 or not wc.is_contiguous():
            wc = wc.float().contiguous()
        L.check(lib.bpx_pack_weight(mode, wc.data_ptr(), cin, cout, self.pdt, out.data_ptr(), L.stream_ptr()))
        if cache:
            self._pack_cache[key] = out
            self._pack_versions[key] = stamp
        return out

    def _pack_image16(self, x: torch.Tensor, st) -> torch.Tensor:
        """x: the (B, C, D, H, W) fp32 image of a zero-padded-input network (NetConfig.true_in_ch), planar or the channels-last view
        to_pytorch_format and the sliding-window predictor pass -> the dense (B, D, H, W, 16) tensor of the storage type the first block
        reads (bpx_image_pack16: one pass, the conversion included).  Any other stride pattern is made planar first."""
        B, Cin, D, H, W = x.shape
        vox = D * H * W
        if x.permute(0, 2, 3, 4, 1).is_contiguous():
            sv, sc = Cin, 1
        else:
            x, sv, sc = x.contiguous(), 1, vox
        out = torch.empty((B, D, H, W, 16), dtype=self.dtype, device=x.device)
        L.check(lib.bpx_image_pack16(self.dt, B, vox, Cin, x.data_ptr(), Cin * vox, sv, sc, out.data_ptr(), st))
        return out

    # ------------------------------------------------------------------------------------------
    def _res_block_fwd(self, P, blk: _Blk, B, img: Optional[torch.Tensor], st, cache: bool, want_out_stats: bool, pool=None):
        """Runs one residual block. Returns partial stats (part, tiles) of the block output if requested.
        pool = (z stride, pooled tensor, its partial-statistics tensor): fuse the MaxPool3d that follows an encoder block into
        the epilogue of the block's last convolution (bpx_conv3d_fwd_pool; the caller checked that it is supported)."""
        D, H, W = blk.S
        dev = blk.out.device
        k = blk.keys
        vox = D * H * W
        C1 = blk.cout
        stats = self._bn_eval is None          # eval-mode BN takes its records from the running buffers: the producers get null statistics pointers
        # ---- conv1 -> h (+ stats) ----------------------------------------------------------------
        if blk.first and self.cfg.in_ch == 1:
            tiles = lib.bpx_conv3d_c1_stats_tiles(D, H, W)
            part = _Stats.alloc(B, tiles, C1, dev) if stats else None
            L.check(lib.bpx_conv3d_c1_fwd(self.dt, B, D, H, W, img.data_ptr(), P[k["w1"]].data_ptr(), P[k["b1"]].data_ptr(),
                                          L.tview(blk.h), L.ptr(part), st))
        else:
            tiles = lib.bpx_conv3d_stats_tiles(self.dt, B, D, H, W, C1)
            part = _Stats.alloc(B, tiles, C1, dev) if stats else None
            wp = self._pack(P[k["w1"]], L.PK_K3, blk.cin, C1, cache)
            L.check(lib.bpx_conv3d_fwd(self.dt, B, D, H, W, L.tview(blk.x, blk.x_c0, blk.cin),
                                       L.ptr(blk.rec_x), self.act if blk.rec_x is not None else 0, wp.data_ptr(), P[k["b1"]].data_ptr(),
                                       L.NULL_T, None, None, L.tview(blk.h), L.ptr(part), st))
        blk.rec_h = self._norm_records(P, k["g1"][:-len(".weight")], part, tiles, C1, vox, st)
        # ---- dropout: conv2 reads the materialised, masked activation instead of forming it in its prologue -------
        x2, rec2, act2 = L.tview(blk.h), blk.rec_h.data_ptr(), self.act
        if blk.drop_p > 0.0 and self.drop_active:
            # THIS forward's counter value (a device copy taken in forward(): capture-safe), kept with the block so that the backward of this pass
            # regenerates this pass's masks even when another forward ran in between (two forwards before one backward, retained graphs)
            ctr = blk.drop_ctr = self._drop_ctr_cur
            blk.a = torch.empty_like(blk.h)
            mptr, mmode = self._drop_mask(blk, blk.h.numel(), dev)
            L.check(lib.bpx_norm_act_dropout_fwd(self.dt, B, vox, L.tview(blk.h), blk.rec_h.data_ptr(), self.act, blk.drop_p, self.drop_seed, ctr.data_ptr(),
                                                 blk.site, mptr, mmode, L.tview(blk.a), st))
            x2, rec2, act2 = L.tview(blk.a), None, 0
        # ---- conv2 (+ shortcut, + residual add) -> out (+ stats) ----------------------------------
        wp2 = self._pack(P[k["w2"]], L.PK_K3, C1, C1, cache)
        tiles2 = lib.bpx_conv3d_stats_tiles(self.dt, B, D, H, W, C1)
        part2 = _Stats.alloc(B, tiles2, C1, dev) if want_out_stats else None
        if blk.first and self.cfg.in_ch == 1:
            sc = L.Tensor(img.data_ptr(), 1, 1)
            wsc_ptr = P[k["wsc"]].data_ptr()  # (Cout,1,1,1,1) fp32 used as a vector
        else:
            sc = L.tview(blk.x, blk.x_c0, blk.cin)
            wsc_ptr = self._pack(P[k["wsc"]], L.PK_K1, blk.cin, C1, cache).data_ptr()
        if pool is not None:
            L.check(lib.bpx_conv3d_fwd_pool(self.dt, B, D, H, W, x2, rec2, act2, wp2.data_ptr(),
                                            P[k["b2"]].data_ptr(), sc, wsc_ptr, P[k["bsc"]].data_ptr(),
                                            L.tview(blk.out, blk.out_c0, C1), L.ptr(part2), pool[0], L.tview(pool[1]), L.ptr(pool[2]), st))
        else:
            L.check(lib.bpx_conv3d_fwd(self.dt, B, D, H, W, x2, rec2, act2, wp2.data_ptr(),
                                       P[k["b2"]].data_ptr(), sc, wsc_ptr, P[k["bsc"]].data_ptr(),
                                       L.tview(blk.out, blk.out_c0, C1), L.ptr(part2), st))
        return part2, tiles2

    # ------------------------------------------------------------------------------------------
    def _level_shapes(self, S0, zd) -> List[Tuple[int, int, int]]:
        """(D, H, W) of every level of a patch S0: z_down zd[i] and y / x down 2 from level i to i + 1."""
        Lv = len(zd)
        zdiv = math.prod(zd)
        if S0[0] % zdiv or S0[1] % (2 ** Lv) or S0[2] % (2 ** Lv):
            raise ValueError(f"patch {tuple(S0)} must be divisible by {(zdiv, 2 ** Lv, 2 ** Lv)} (DATA.PATCH_SIZE rule, check_configuration.py:3156-3202)")
        S = [tuple(S0)]
        for i in range(Lv):
            S.append((S[i][0] // zd[i], S[i][1] // 2, S[i][2] // 2))
        return S

    def _ingest(self, x: torch.Tensor, x_ndhwc: Optional[torch.Tensor], st):
        """The (B, C, D, H, W) fp32 image as the first block reads it -> (img, x_ndhwc): one channel as the planar fp32 img; otherwise a dense NDHWC
        tensor of the storage type - the caller's own, the zero-padded 16 channels of a 2 to 15 channel image (_pack_image16), or a cast copy."""
        B, Cin, D0, H0, W0 = x.shape
        if Cin == 1:
            return x.reshape(B, D0, H0, W0).contiguous(), None
        if x_ndhwc is not None:
            return None, x_ndhwc
        if self.cfg.true_in_ch is not None:
            return None, self._pack_image16(x, st)
        xin = x.permute(0, 2, 3, 4, 1).contiguous()
        x_ndhwc = torch.empty(xin.shape, dtype=self.dtype, device=x.device)
        if self.dtype == torch.float32:
            x_ndhwc.copy_(xin)
        else:
            L.check(lib.bpx_cast(L.F32, xin.data_ptr(), self.dt, x_ndhwc.data_ptr(), xin.numel(), st))
        return None, x_ndhwc

    def forward(self, P: Dict[str, torch.Tensor], x: Optional[torch.Tensor], head_act: int = 0, save: bool = False, cache_weights: bool = False,
                x_ndhwc: Optional[torch.Tensor] = None, want_dx: bool = False):
        """x: (B,C,Z,Y,X) fp32 with channels_last_3d strides (or any layout for C == 1; planar or channels-last for the 2 to 15 channels of a
        zero-padded image, NetConfig.true_in_ch).  Returns logits
        (B,sum(out_ch),Z,Y,X) fp32 in channels-first planar layout, and the saved context (or None).
        ``x_ndhwc``: the input already as a dense (B,Z,Y,X,C) tensor of the storage dtype (``x`` is then ignored); ``want_dx``: the
        backward also returns the gradient of that tensor under the key "__dx__" (super-resolution pre-up-sampling, resunet_sr)."""
        cfg = self.cfg
        if x_ndhwc is not None:
            assert x_ndhwc.is_cuda and x_ndhwc.dtype == self.dtype and x_ndhwc.dim() == 5 and x_ndhwc.is_contiguous() and cfg.in_ch != 1
            x = x_ndhwc.permute(0, 4, 1, 2, 3)           # only its shape is used below
        else:
            assert x.is_cuda and x.dtype == torch.float32 and x.dim() == cfg.ndim + 2
        groups = self._groups_for(x.shape[0], ((1,) + tuple(x.shape[2:]))[-3:], save)
        if len(groups) > 1:
            return self._forward_groups(groups, lambda **a: self.forward(P, head_act=head_act, cache_weights=cache_weights, want_dx=want_dx, **a),
                                        x, save, x_ndhwc=x_ndhwc)
        if cfg.ndim == 2:
            x = x.unsqueeze(2)
        if self.drop_active and any(v > 0 for v in cfg.dropout):
            # a new mask per forward pass (a device value: replayed graphs advance it too); the pass works from its own snapshot
            self._drop_ctr_cur = self._drop_state(x.device).add_(1).clone()
        P_orig = P
        if cache_weights and torch.cuda.is_current_stream_capturing():
            # a captured forward must contain its own pack kernels: operands cached during the warm-up would freeze the
            # weights of every later replay at their capture-time values (graphs.GraphedInference)
            cache_weights = False
        self._bn_eval = None
        if self.bn:
            if not self.bn_training:
                self._bn_eval = self._bn_eval_records(P, x.shape[0], x.device, cache_weights)
            else:
                self._bn_steps += 1
        plan = self._pad_plan
        if plan is not None or cfg.true_in_ch is not None or any(needs_lift(w) for w in P.values()):
            # 2D / anisotropic levels: zero-padded 3x3x3 weights.  Inference keeps the lifted copies while the parameters
            # are unchanged, so that the packed-operand cache (keyed by storage) keeps hitting.
            vers = (_WEIGHTS_EPOCH[0],) + tuple((w.data_ptr(), w._version) for w in P.values())
            hit = getattr(self, "_lift_cache", None)
            if cache_weights and hit is not None and hit[0] == vers:
                P = hit[1]
            else:
                P = P if plan is None else pad_channels(P, plan)
                P = lift_params(P if cfg.true_in_ch is None else pad_input_channels(P, cfg.in_ch))
                self._lift_cache = (vers, P) if cache_weights else None
        B, Cin, D0, H0, W0 = x.shape
        assert Cin == (cfg.true_in_ch or cfg.in_ch), f"expected {cfg.true_in_ch or cfg.in_ch} input channels, got {Cin}"
        Lv = cfg.depth
        S = self._level_shapes((D0, H0, W0), cfg.z_down)
        dev = x.device
        st = L.stream_ptr()
        fm = list(cfg.feature_maps)
        T = self.dtype
        if not cache_weights:
            self._prepack(P, save, dev)       # ONE batched pack launch (training re-packs every step; so does a captured inference)
        else:
            self._prepacked = {}
        img, x_ndhwc = self._ingest(x, x_ndhwc, st)
        if self.bn and self.bn_training and B * S[Lv][0] * S[Lv][1] * S[Lv][2] == 1:
            # what torch.nn.functional.batch_norm raises (at the bottleneck's first norm, the first with one value per channel); up front, not from a kernel
            raise ValueError(f"Expected more than 1 value per channel when training, got input size torch.Size([{B}, {fm[Lv - 1]}, 1, 1, 1])")

        def buf(i, C):
            return torch.empty((B,) + S[i] + (C,), dtype=T, device=dev)

        # torch.cat([up, skip], 1) buffers, chunk-planar (L.Planar): the transposed conv and the encoder block write whole planes
        # instead of 64 / 32 of every 96 bytes, pooling reads a dense plane
        cat = [L.Planar(B, S[i], fm[i + 1] + fm[i], T, dev) for i in range(Lv)]
        blocks: List[_Blk] = []
        pools = []
        out_stats = []
        cur, cur_rec = x_ndhwc, None
        # ---------------- encoder ------------------------------------------------------------------
        for i in range(Lv):
            blk = _Blk(keys=block_keys(f"down_path.{i}", i == 0), first=(i == 0), S=S[i], cin=(cfg.in_ch if i == 0 else fm[i - 1]),
                       cout=fm[i], x=cur, x_c0=0, rec_x=cur_rec, h=buf(i, fm[i]), out=cat[i], out_c0=fm[i + 1], drop_p=cfg.dropout[i], site=i)
            # pool -> P_i (+ stats) and the pre-norm record of the next block; fused into the block's last conv where the
            # lean kernel runs (>= 64^3 levels, bf16): the output slice is then not read again
            pooled = buf(i + 1, fm[i])
            D, H, W = S[i]
            k_ = blk.keys
            fused = bool(lib.bpx_conv3d_fwd_pool_supported(self.dt, B, D, H, W, fm[i], cat[i].shape[-1], fm[i])) and all(
                P[k_[q]].data_ptr() % 16 == 0 for q in ("b2", "bsc", "wsc"))
            stats = self._bn_eval is None
            if fused:
                ptiles = lib.bpx_conv3d_stats_tiles(self.dt, B, D, H, W, fm[i])
                ppart = _Stats.alloc(B, ptiles, fm[i], dev) if stats else None
                part, tiles = self._res_block_fwd(P, blk, B, img, st, cache_weights, want_out_stats=stats, pool=(cfg.z_down[i], pooled, ppart))
            else:
                part, tiles = self._res_block_fwd(P, blk, B, img, st, cache_weights, want_out_stats=stats)
                ptiles = lib.bpx_maxpool3d_stats_tiles(self.dt, D, H, W, cfg.z_down[i], fm[i])
                ppart = _Stats.alloc(B, ptiles, fm[i], dev) if stats else None
                L.check(lib.bpx_maxpool3d_fwd(self.dt, B, D, H, W, cfg.z_down[i], L.tview(cat[i], fm[i + 1], fm[i]), L.tview(pooled), L.ptr(ppart), st))
            out_stats.append((part, tiles))
            blocks.append(blk)
            nxt = "bottleneck" if i == Lv - 1 else f"down_path.{i + 1}"
            pools.append(pooled)
            cur, cur_rec = pooled, self._norm_records(P, f"{nxt}.block.0", ppart, ptiles, fm[i], math.prod(S[i + 1]), st)
        # ---------------- bottleneck ----------------------------------------------------------------
        bot = _Blk(keys=block_keys("bottleneck", False), first=False, S=S[Lv], cin=fm[Lv - 1], cout=fm[Lv], x=cur, rec_x=cur_rec,
                   h=buf(Lv, fm[Lv]), out=buf(Lv, fm[Lv]), out_c0=0, drop_p=cfg.dropout[Lv], site=Lv)
        self._res_block_fwd(P, bot, B, img, st, cache_weights, want_out_stats=False)
        blocks.append(bot)
        # ---------------- decoder -------------------------------------------------------------------
        dec_in = bot.out
        ups = []
        for j, i in enumerate(range(Lv - 1, -1, -1)):
            Cup = fm[i + 1]
            Dl, Hl, Wl = S[i + 1]
            wk, bk = f"up_paths.0.{j}.up.weight", f"up_paths.0.{j}.up.bias"
            szl = cfg.z_down[i]
            wp = self._pack(P[wk], L.PK_CT if szl == 2 else L.PK_CT4, Cup, Cup, cache_weights)
            utiles = lib.bpx_convT3d_stats_tiles(Dl, Hl, Wl, szl)
            upart = _Stats.alloc(B, utiles, Cup, dev) if self._bn_eval is None else None
            L.check(lib.bpx_convT3d_k2s2_fwd(self.dt, B, Dl, Hl, Wl, szl, L.tview(dec_in), wp.data_ptr(), P[bk].data_ptr(),
                                             L.tview(cat[i], 0, Cup), L.ptr(upart), st))
            pre = f"up_paths.0.{j}.conv_block"
            rec = self._cat_records(P, f"{pre}.block.0", [(upart, utiles, Cup), out_stats[i] + (fm[i],)], B, math.prod(S[i]), dev, st)
            blk = _Blk(keys=block_keys(pre, False), first=False, S=S[i], cin=Cup + fm[i], cout=fm[i], x=cat[i], x_c0=0, rec_x=rec,
                       h=buf(i, fm[i]), out=buf(i, fm[i]), out_c0=0, drop_p=cfg.dropout[i], site=Lv + 1 + j)
            self._res_block_fwd(P, blk, B, img, st, cache_weights, want_out_stats=False)
            blocks.append(blk)
            ups.append((wk, bk, dec_in, Cup, S[i + 1], szl))
            dec_in = blk.out
        # ---------------- heads ----------------------------------------------------------------------
        hw, hb = self._head_matrix(P)
        feat, So = dec_in, (D0, H0, W0)
        if cfg.post_up:
            # super-resolution: ConvTranspose3d(fm0, fm0, k = s = (post_up, 2, 2)) on the decoder output (resunet.py:399-400)
            So = (D0 * cfg.post_up, H0 * 2, W0 * 2)
            wpu = self._pack(P["post_upsampling.weight"], L.PK_CT if cfg.post_up == 2 else L.PK_CT4, fm[0], fm[0], cache_weights)
            feat = torch.empty((B,) + So + (fm[0],), dtype=T, device=dev)
            pupart = _Stats.alloc(B, lib.bpx_convT3d_stats_tiles(D0, H0, W0, cfg.post_up), fm[0], dev)       # statistics unused
            L.check(lib.bpx_convT3d_k2s2_fwd(self.dt, B, D0, H0, W0, cfg.post_up, L.tview(dec_in), wpu.data_ptr(), P["post_upsampling.bias"].data_ptr(),
                                             L.tview(feat), pupart.data_ptr(), st))
        logits, wide = self._head_fwd(B, So, feat, hw, hb, head_act, st, dev)
        if cfg.ndim == 2:
            logits = logits.reshape(B, -1, So[1], So[2])
        ctx = None
        if save:
            ctx = dict(B=B, S=S, So=So, img=img, x_ndhwc=x_ndhwc, blocks=blocks, cat=cat, pools=pools, ups=ups, feat=feat, dec_out=dec_in, hw=hw,
                       Pw=(P if P is not P_orig else None), want_dx=want_dx, wide_head=wide, bn_running=self._bn_eval is not None,
                       prepacked=self._prepacked)
        return logits, ctx

    # ------------------------------------------------------------------------------------------
    def _block_bwd(self, P, G, blk: _Blk, B, dOut: L.Tensor, img, st, dx_out=None, r1_done: bool = False):
        """Backward of one residual block.  dOut: gradient of the block output (T, NDHWC view).
        Writes parameter grads into G; writes the input gradient into dx_out: a view with blk.cin channels, a decoder block's (up, skip) pair of
        views, or None when the input needs none.  r1_done: the first block's shortcut weight gradient was formed by bpx_maxpool3d_bwd_r1, the
        pass that wrote dOut (see _backward)."""
        D, H, W = blk.S
        k, dev, C1, Cx, vox = blk.keys, blk.h.device, blk.cout, blk.cin, D * H * W
        first_c1 = blk.first and self.cfg.in_ch == 1
        hv = L.tview(blk.h)
        xv = None if first_c1 else L.tview(blk.x, blk.x_c0, Cx)
        # ---- conv2: weight / bias gradients (both biases add to the same tensor: identical gradients, written by the same reduction) --------------
        dropped = blk.a is not None                      # training-mode dropout: conv2 read the materialised, masked activation blk.a
        fused2 = not dropped and self._bwd_fused_ok(B, blk.S, C1, dOut.C)
        if dropped:
            self._wgrad(B, blk.S, L.tview(blk.a), None, 0, dOut, 3, G[k["w2"]], G[k["b2"]], st, dev, db2=G[k["bsc"]])
        elif not fused2:
            self._wgrad(B, blk.S, hv, blk.rec_h, self.act, dOut, 3, G[k["w2"]], G[k["b2"]], st, dev, db2=G[k["bsc"]])
        # ---- shortcut weight gradient.  Decoder blocks at the large levels: it rides along in the pass that forms the block's input gradient
        # (bpx_conv1x1_fwd_split_wgrad below streams both of its operands anyway); everywhere else it is a launch of its own
        sc_ws = 0
        if (isinstance(dx_out, tuple) and blk.rec_x is not None and self.cfg.gn_groups == 0
                and dOut.C * 3 == Cx and self.dtype != torch.float32):
            # asked with the operands: the kernel's span, pitch and alignment bounds decide too (g0 and coef0 are allocated below, dense)
            sc_ws = int(lib.bpx_conv1x1_fwd_split_wgrad_query(self.bdt, B, vox, dOut, L.Tensor(None, Cx, Cx, 0), xv, None, dx_out[0], dx_out[1]))
        if first_c1:
            if not r1_done:
                ws1 = self._workspace(lib.bpx_conv1x1_c1_wgrad_workspace(C1), dev)
                L.check(lib.bpx_conv1x1_c1_wgrad(self.gdt, B * vox, img.data_ptr(), dOut, G[k["wsc"]].data_ptr(), ws1.data_ptr(), ws1.numel(), st))
        elif not sc_ws:
            self._wgrad(B, blk.S, xv, None, 0, dOut, 1, G[k["wsc"]], None, st, dev)
        # ---- conv2: input gradient, times act' (and the dropout mask), with the reduction partials of the h norm ---------------------------------
        g1 = torch.empty((B, D, H, W, C1), dtype=self.gdtype, device=dev)
        self._keep.append(g1)
        gv = L.tview(g1)
        w2t = self._pack(P[k["w2"]], L.PK_K3_T, C1, C1, False)
        if dropped:   # plain dgrad -> gradient of the masked activation; then mask, activation derivative and the IN-backward sums in one pass
            L.check(lib.bpx_conv3d_dgrad(self.gdt, B, D, H, W, dOut, w2t.data_ptr(), L.NULL_T, None, 0, gv, None, st))
            tiles = lib.bpx_norm_act_dropout_tiles(self.gdt, vox, C1)
            red = torch.empty((B, tiles, 2, C1), dtype=torch.float32, device=dev)
            mptr, mmode = self._drop_mask(blk, g1.numel(), dev)
            L.check(lib.bpx_norm_act_dropout_bwd(self.bdt, B, vox, gv, hv, blk.rec_h.data_ptr(), self.act, blk.drop_p, self.drop_seed,
                                                 blk.drop_ctr.data_ptr(), blk.site, mptr, 1 if mmode else 0, gv, red.data_ptr(), st))
        else:
            tiles, red = self._dgrad_prologue(B, blk.S, dOut, w2t, hv, blk.rec_h, self.act, gv, st, fused=fused2,
                                              dw=G[k["w2"]], db=G[k["b2"]], db2=G[k["bsc"]])
        coef = self._norm_bwd_coef(red, B, tiles, C1, vox, blk.rec_h, P[k["g1"]], G[k["g1"]], G[k["be1"]], st, deferred=True)
        # ---- dH = a * g1 + b * h + c0 in place; the first layer (no input gradient) leaves with its weight gradient ----------------------------
        if first_c1:
            # where the kernel takes the width, dH is formed inside the weight-gradient kernel, its only reader, and never stored
            nb = lib.bpx_conv3d_c1_wgrad_nb_supported(self.bdt, W)
            if not nb:
                L.check(lib.bpx_norm_bwd_apply(self.bdt, B, vox, gv, hv, coef.data_ptr(), L.NULL_T, gv, st))
            wsc = self._workspace(lib.bpx_conv3d_c1_wgrad_workspace(C1), dev)
            if nb:
                self._keep.append(coef)
                L.check(lib.bpx_conv3d_c1_wgrad_nb(self.bdt, B, D, H, W, img.data_ptr(), gv, hv, coef.data_ptr(), G[k["w1"]].data_ptr(),
                                                   G[k["b1"]].data_ptr(), wsc.data_ptr(), wsc.numel(), st))
            else:
                L.check(lib.bpx_conv3d_c1_wgrad(self.gdt, B, D, H, W, img.data_ptr(), gv, G[k["w1"]].data_ptr(), G[k["b1"]].data_ptr(),
                                                wsc.data_ptr(), wsc.numel(), st))
            return
        L.check(lib.bpx_norm_bwd_apply(self.bdt, B, vox, gv, hv, coef.data_ptr(), L.NULL_T, gv, st))
        # ---- conv1: weight / bias gradients; with a wanted dx the input gradient g0 and the reduction partials of the x norm -------------------
        has_norm = blk.rec_x is not None
        fused1 = has_norm and dx_out is not None and self._bwd_fused_ok(B, blk.S, Cx, C1)
        if not fused1:
            self._wgrad(B, blk.S, xv, blk.rec_x, self.act if has_norm else 0, gv, 3, G[k["w1"]], G[k["b1"]], st, dev)
        if dx_out is None:
            return
        g0 = torch.empty((B, D, H, W, Cx), dtype=self.gdtype, device=dev)
        w1t = self._pack(P[k["w1"]], L.PK_K3_T, Cx, C1, False)
        wsct = self._pack(P[k["wsc"]], L.PK_DENSE_T, Cx, C1, False)
        if not has_norm:      # a first block that reads a dense tensor (16 channels and up): dx = dgrad + shortcut, no norm in between
            L.check(lib.bpx_conv3d_dgrad(self.gdt, B, D, H, W, gv, w1t.data_ptr(), L.NULL_T, None, 0, L.tview(g0), None, st))
            L.check(lib.bpx_conv1x1_fwd(self.gdt, B, vox, dOut, wsct.data_ptr(), None, L.NULL_T, L.NULL_T, None, L.tview(g0), dx_out, st))
            return
        tiles0, red0 = self._dgrad_prologue(B, blk.S, gv, w1t, xv, blk.rec_x, self.act, L.tview(g0), st, fused=fused1, dw=G[k["w1"]], db=G[k["b1"]])
        coef0 = self._norm_bwd_coef(red0, B, tiles0, Cx, vox, blk.rec_x, P[k["g0"]], G[k["g0"]], G[k["be0"]], st, deferred=True)
        # ---- hand-over: dx = a0 * g0 + b0 * x + c0 + shortcut^T dOut in one pointwise pass; a decoder block's leaves as its (up, skip) parts ----
        if not isinstance(dx_out, tuple):
            L.check(lib.bpx_conv1x1_fwd(self.bdt, B, vox, dOut, wsct.data_ptr(), None, L.tview(g0), xv, coef0.data_ptr(), L.NULL_T, dx_out, st))
        elif sc_ws:
            wsw = self._workspace(sc_ws, dev)
            L.check(lib.bpx_conv1x1_fwd_split_wgrad(self.bdt, B, vox, dOut, wsct.data_ptr(), L.tview(g0), xv, coef0.data_ptr(), dx_out[0], dx_out[1],
                                                    G[k["wsc"]].data_ptr(), wsw.data_ptr(), wsw.numel(), st))
        else:
            L.check(lib.bpx_conv1x1_fwd_split(self.bdt, B, vox, dOut, wsct.data_ptr(), None, L.tview(g0), xv, coef0.data_ptr(),
                                              L.NULL_T, dx_out[0], dx_out[1], st))

    def backward(self, P: Dict[str, torch.Tensor], ctx, dlogits: torch.Tensor, on_last_block=None) -> Dict[str, torch.Tensor]:
        """``on_last_block``: called (no arguments) right before the backward of the FIRST encoder block - the last stretch of the pass.  At that
        point every queued weight-gradient reduction has been flushed, so all parameter gradients except ``down_path.0.*`` are final in the flat
        slab (``self.last_flat_grad``, parameter order): a data-parallel step starts their all-reduce there and lets it run beside the rest of
        the backward (graphs.DataParallelTrainStep; what DDP's buckets do for the reference, base_workflow.py:952-958).  A batch that ran as
        several sample groups (batch_groups) calls it once, after the last group: only then are the summed gradients final."""
        if ctx is not None and "groups" in ctx:
            return self._backward_groups(ctx, dlogits, lambda c, d: self.backward(P, c, d), on_last_block)
        self._prepacked = ctx["prepacked"]                          # the packed operands of this context's own forward
        Pw = ctx.get("Pw")
        self._bn_running = int(ctx.get("bn_running", False))      # BatchNorm: the forward normalised with the running statistics (eval mode)
        # the ~29 weight-gradient reductions of a step run as one batched launch at the end (they are latency chains of a
        # few hundred blocks each; back to back they cost 0.6 ms)
        with self._backward_pass(defer=True):
            G = self._backward(P if Pw is None else Pw, ctx, dlogits, on_last_block)
        if Pw is None:
            return G
        if self._pad_plan is not None:                        # zero-padded widths: the parameters' own rows / columns of the padded gradients
            G = unpad_channel_grads(G, self._pad_plan)
        if self.cfg.true_in_ch is not None:                   # zero-padded image: the real input channels' columns of the first block's two weights
            G = unpad_input_grads(G, self.cfg.true_in_ch)
        return unlift_grads(G, P)                            # after the flush: it is the flush that writes the conv gradients

    def _backward(self, P: Dict[str, torch.Tensor], ctx, dlogits: torch.Tensor, on_last_block) -> Dict[str, torch.Tensor]:
        cfg = self.cfg
        B, S, img = ctx["B"], ctx["S"], ctx["img"]
        blocks: List[_Blk] = ctx["blocks"]
        cat, pools, ups, feat = ctx["cat"], ctx["pools"], ctx["ups"], ctx["feat"]
        fm = list(cfg.feature_maps)
        Lv = cfg.depth
        dev = dlogits.device
        st = L.stream_ptr()
        T = self.gdtype
        G = self._grad_slab(P, dev)
        # ---- head -------------------------------------------------------------------------------
        So = tuple(ctx.get("So", S[0]))
        dfeat = torch.empty((B,) + So + (fm[0],), dtype=T, device=dev)
        self._head_bwd(G, B, So, L.tview(feat), ctx["hw"], dlogits.contiguous().float(), L.tview(dfeat), st, dev, wide=ctx.get("wide_head"))
        self._keep.append(dfeat)
        if cfg.post_up:
            dfeat = self._convT_bwd(P, G, B, S[0], cfg.post_up, ctx["dec_out"], dfeat, "post_upsampling.weight", "post_upsampling.bias", fm[0], fm[0], st, dev)
        # ---- decoder (blocks list: enc 0..Lv-1, bottleneck, dec j=0..Lv-1 for levels Lv-1..0) -------
        dskip: List[Optional[torch.Tensor]] = [None] * Lv      # d(concat) leaves the decoder block as two dense tensors
        dOut = dfeat
        for j in range(Lv - 1, -1, -1):       # decoder block j handles level i = Lv-1-j; walk from level 0 up
            i = Lv - 1 - j
            wk, bk, x_in, Cup, Sl, szl = ups[j]
            dup = torch.empty((B,) + S[i] + (Cup,), dtype=T, device=dev)
            dskip[i] = torch.empty((B,) + S[i] + (fm[i],), dtype=T, device=dev)
            self._block_bwd(P, G, blocks[Lv + 1 + j], B, L.tview(dOut), img, st, (L.tview(dup), L.tview(dskip[i])))
            dOut = self._convT_bwd(P, G, B, Sl, szl, x_in, dup, wk, bk, Cup, Cup, st, dev)
        # ---- bottleneck -------------------------------------------------------------------------
        dP = torch.empty((B,) + S[Lv] + (fm[Lv - 1],), dtype=T, device=dev)
        self._block_bwd(P, G, blocks[Lv], B, L.tview(dOut), img, st, L.tview(dP))
        # ---- encoder ------------------------------------------------------------------------------
        for i in range(Lv - 1, -1, -1):
            D, H, W = S[i]
            Cup = fm[i + 1]
            # dOut_i = dSkip + unpool(dP); written in place over dSkip
            skipv = L.tview(dskip[i])
            r1_ws = 0
            if i == 0 and cfg.in_ch == 1 and self.dtype != torch.float32:
                # level 0 of a one-channel-image network (round 6): the first block's rank-1 shortcut weight gradient is a sum over the tensor this pass writes
                r1_ws = int(lib.bpx_maxpool3d_bwd_r1_workspace(self.bdt, B, D, H, W, cfg.z_down[i], fm[i]))
            if r1_ws:
                wsr = self._workspace(r1_ws, dev)
                L.check(lib.bpx_maxpool3d_bwd_r1(self.bdt, B, D, H, W, cfg.z_down[i], L.tview(cat[i], Cup, fm[i]), L.tview(dP), skipv, skipv, img.data_ptr(),
                                                 G[blocks[0].keys["wsc"]].data_ptr(), wsr.data_ptr(), wsr.numel(), st))
            else:
                L.check(lib.bpx_maxpool3d_bwd(self.bdt, B, D, H, W, cfg.z_down[i], L.tview(cat[i], Cup, fm[i]), L.tview(dP), skipv, skipv, st))
            if i == 0 and on_last_block is not None:
                # the reductions queued so far write their gradients now; the last block's are queued afresh
                L.check(lib.bpx_wgrad_defer_flush(L.stream_ptr()))
                L.check(lib.bpx_wgrad_defer_begin())
                on_last_block()
            if i > 0:
                dPn = torch.empty((B,) + S[i] + (fm[i - 1],), dtype=T, device=dev)
                self._block_bwd(P, G, blocks[i], B, skipv, img, st, L.tview(dPn))
                self._keep.append(dP)
                dP = dPn
            elif ctx.get("want_dx"):
                dx0 = torch.empty((B,) + S[0] + (cfg.in_ch,), dtype=T, device=dev)
                self._block_bwd(P, G, blocks[0], B, skipv, img, st, L.tview(dx0), r1_done=bool(r1_ws))
                G["__dx__"] = dx0
            else:
                self._block_bwd(P, G, blocks[0], B, skipv, img, st, None, r1_done=bool(r1_ws))  # the image needs no gradient
        return G
