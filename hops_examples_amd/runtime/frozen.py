"""Frozen ResNet inference: BatchNorm folded into the convs, the residual added in the conv epilogue.

At inference a BatchNorm is a constant per-channel affine, so every ``ConvBN`` of models/resnet.py is ONE
conv launch here: the BN's scale goes into the weight, its shift into a bias, and the block's last conv
adds the shortcut before the ReLU in its own epilogue (kernels.conv2d_fwd_res) — where the training graph
in ``eval()`` mode runs a conv launch that stores a rounded bf16 tensor and a ``bn_fwd_infer`` launch that
re-reads it.  ResNet-20: 45 -> 24 launches per forward, ResNet-50: 110 -> 57 (counts derived from the model
definitions), and one full read + write of every activation tensor less.

* ``fold_conv_bn``      the fold itself, dtype-generic pure torch (the engine and the fp64 reference share it)
* ``FrozenResNet``      the GPU engine (``Predictor(frozen=...)`` routes to it)
* ``reference_forward`` the same structure in any dtype on any device, optionally rounding exactly what the
                        engine stores as bf16
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ..models.resnet import BasicBlock, CifarResNet, ConvBN, ResNet50, _as_nhwc_image
from ..ops import functional as HF
from ..ops import kernels as K

BF16 = torch.bfloat16


def fold_conv_bn(w, gamma, beta, rmean, rvar, eps):
    """(w', b') with conv(x, w') + b' == bn(conv(x, w)) for an inference BatchNorm: s = gamma / sqrt(rvar + eps),
    w' = w * s[co] (the output channel is w's first axis), b' = beta - rmean * s.  Computed in the dtype of the
    arguments."""
    s = gamma / torch.sqrt(rvar + eps)
    return w * s.reshape(-1, *([1] * (w.dim() - 1))), beta - rmean * s


def _layers(model):
    """[(name, ConvBN)] in module order."""
    return [(n, m) for n, m in model.named_modules() if isinstance(m, ConvBN)]


def _run_structure(model, x, layer, maxpool):
    """The ResNets' data flow over ``layer(name, convbn, x, residual) -> y``: the block's last conv takes the
    shortcut as its residual (act(bn(conv) + shortcut))."""
    y = layer("stem", model.stem, x, None)
    if isinstance(model, ResNet50):
        y = maxpool(y)
    for i, blk in enumerate(model.blocks):
        p = f"blocks.{i}."
        s = y if blk.short is None else layer(p + "short", blk.short, y, None)
        h = layer(p + "a", blk.a, y, None)
        if isinstance(blk, BasicBlock):
            y = layer(p + "b", blk.b, h, s)
        else:
            y = layer(p + "c", blk.c, layer(p + "b", blk.b, h, None), s)
    return y


class FrozenResNet:
    """Inference engine of a ``CifarResNet`` / ``ResNet50`` on a GPU: one conv launch per ``ConvBN``.

    The object is a SNAPSHOT of the model's conv weights and BatchNorm state taken by ``freeze`` (folded from
    the fp32 master weights, rounded to bf16 once).  Later changes to the model (training steps, a loaded
    checkpoint) are not seen until ``refresh()``, which refolds INTO THE SAME BUFFERS — graphs captured over
    ``__call__`` stay valid and replay the new state.  Staleness between ``refresh()`` calls is the caller's
    business.  The classifier weights, the max-pool and the global average pool are the model's own and are
    always current."""

    def __init__(self, model):
        if not self.supported(model):
            raise ValueError("FrozenResNet: a CifarResNet / ResNet50 on a GPU is required")
        self.model = model
        self.layers = _layers(model)
        self._w, self._b, self._cfg = {}, {}, {}
        dev = next(model.parameters()).device
        for name, m in self.layers:
            co, kh, kw, ci = m.conv.weight.shape
            self._w[name] = torch.empty(co, kh, kw, ci, device=dev, dtype=BF16)
            self._b[name] = torch.empty(co, device=dev, dtype=torch.float32)
            self._cfg[name] = (int(m.conv.cfg["stride"]), int(m.conv.cfg["padding"]), HF.ACT[m.bn.activation])
        # the stem weight zero-padded to the 8 channels the uint8 normaliser writes (the 3-channel copy above
        # serves HOPSX_DISABLE=stem_pad and float inputs)
        co, kh, kw, _ = model.stem.conv.weight.shape
        self._w_pad = torch.zeros(co, kh, kw, 8, device=dev, dtype=BF16)
        self.refresh()

    @staticmethod
    def supported(model) -> bool:
        if not isinstance(model, (CifarResNet, ResNet50)):
            return False
        p = next(model.parameters(), None)
        return p is not None and p.is_cuda

    @classmethod
    def freeze(cls, model) -> "FrozenResNet":
        return cls(model)

    @torch.no_grad()
    def refresh(self) -> None:
        """Refold the model's current conv weights and BatchNorm state into the existing buffers."""
        for name, m in self.layers:
            bn = m.bn
            w, b = fold_conv_bn(m.conv.weight.detach().float(), bn.weight.detach().float(), bn.bias.detach().float(),
                                bn.running_mean.float(), bn.running_var.float(), float(bn.eps))
            self._w[name].copy_(w)  # fp32 -> bf16, round to nearest even, once
            self._b[name].copy_(b)
        self._w_pad[..., :self._w["stem"].shape[-1]].copy_(self._w["stem"])

    def folded(self, name):
        """(bf16 weight [CO, KH, KW, C], fp32 bias [CO]) the kernels read for layer ``name``."""
        return self._w[name], self._b[name]

    def buffers(self):
        """Every folded buffer (their addresses are stable across ``refresh``)."""
        return [*self._w.values(), *self._b.values(), self._w_pad]

    def _layer(self, rec):
        def layer(name, m, x, residual):
            st, pd, act = self._cfg[name]
            w = self._w[name]
            if x.shape[-1] != w.shape[-1]:
                if name != "stem" or getattr(x, "_hx_chpad", None) != w.shape[-1] or x.shape[-1] != 8:
                    raise ValueError(f"{name}: expects {w.shape[-1]} input channels (NHWC), got {tuple(x.shape)}")
                w = self._w_pad
            g = K.conv_geom(x.shape, w.shape, (st, st), (pd, pd), (1, 1))
            if residual is None:
                y = K.conv2d_fwd(x, w, g, bias=self._b[name], act=act)
            else:
                y = K.conv2d_fwd_res(x, w, g, bias=self._b[name], act=act, residual=residual)
            if rec is not None:
                rec.append((name, x, residual, y))
            return y
        return layer

    @torch.no_grad()
    def _forward(self, x, rec=None):
        m = self.model
        if not x.is_cuda:
            raise ValueError("FrozenResNet runs on the GPU")
        x = _as_nhwc_image(x, m)  # uint8 NHWC: normalised on the device; float: already preprocessed
        x = HF.to_compute(x) if x.dtype != BF16 else x
        y = _run_structure(m, x.contiguous() if not x.is_contiguous() else x, self._layer(rec), m.maxpool
                           if isinstance(m, ResNet50) else None)
        return m.fc(m.pool(y))

    def __call__(self, x):
        """Logits (fp32) for uint8 NHWC images, or for a float tensor that is already preprocessed."""
        return self._forward(x)

    def trace(self, x):
        """One forward; per frozen layer, in execution order, the tensors its kernel read and wrote:
        ``[(name, input, residual or None, output)]``."""
        rec: list = []
        self._forward(x, rec)
        return rec


@torch.no_grad()
def reference_forward(model, x, dtype=torch.float64, emulate_bf16=True):
    """The frozen forward in ``dtype`` with plain torch ops on ``x``'s device: the engine's structure (folded
    convs, the residual before the activation), not its kernels.  ``emulate_bf16`` rounds exactly what the
    engine stores as bf16 — the normalised input, the folded weights, every layer output, the pooled features
    and the classifier weight — so the result differs from the engine's only by the fp32 summation order;
    without it nothing is rounded (the anchor against ``model.double().eval()``)."""
    def rnd(t):
        return t.to(BF16).to(dtype) if emulate_bf16 else t

    if x.dtype == torch.uint8:
        # the normaliser's constants are fp32 kernel arguments
        cdt = torch.float32 if emulate_bf16 else dtype
        sc = torch.tensor(model.img_scale_c, dtype=cdt, device=x.device).to(dtype)
        sh = torch.tensor(model.img_shift_c, dtype=cdt, device=x.device).to(dtype)
        y = x.to(dtype)
        if model.img_reverse:
            y = y.flip(-1)
        y = y * sc + sh
    else:
        y = x.to(dtype)
    y = rnd(y)

    def layer(name, m, xin, residual):
        bn = m.bn
        w, b = fold_conv_bn(m.conv.weight.detach().to(dtype), bn.weight.detach().to(dtype),
                            bn.bias.detach().to(dtype), bn.running_mean.to(dtype), bn.running_var.to(dtype),
                            float(bn.eps))
        st, pd = int(m.conv.cfg["stride"]), int(m.conv.cfg["padding"])
        o = F.conv2d(xin.permute(0, 3, 1, 2), rnd(w).permute(0, 3, 1, 2), b, st, pd).permute(0, 2, 3, 1)
        if residual is not None:
            o = o + residual
        return rnd(HF._cpu_act(o, bn.activation)).contiguous()

    def maxpool(t):
        mp = model.maxpool
        return F.max_pool2d(t.permute(0, 3, 1, 2), mp.k, mp.s, mp.p).permute(0, 2, 3, 1).contiguous()

    y = _run_structure(model, y, layer, maxpool)
    feat = rnd(y.mean(dim=(1, 2)))
    fc = model.fc
    return F.linear(feat, rnd(fc.weight.detach().to(dtype)), None if fc.bias is None else fc.bias.detach().to(dtype))
