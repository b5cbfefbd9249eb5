"""``SegNet`` -- host-side mirror of the reference's segmentation network (vanilla_segmentation/segnet.py:6-121), the
producer of the masks LineMOD evaluation reads (datasets/linemod/dataset.py:57-58).

Kept: ``SegNet(input_nbr=3, label_nbr=22)``, ``forward(x [B,3,H,W]) -> logits [B,label_nbr,H,W]``, and the state-dict
layout (``convXY.{weight,bias}``, ``bnXY.{weight,bias,running_mean,running_var,num_batches_tracked}`` for the 13
encoder and 13 decoder convolutions), so ``model.load_state_dict(torch.load(...))`` works on a reference checkpoint.

Different: the submodules are parameter containers only.  ``eval()`` forward folds every BatchNorm into its convolution
(w' = w g / sqrt(var + eps), b' = (b - mean) g / sqrt(var + eps) + beta), keeps activations channels-last and runs
conv + bias + ReLU as one launch of the fp32-MFMA kernel (the >= 256-channel layers through the Winograd domain), the
2x2 max-pool / un-pool pairs through ``df_maxpool2x2_idx`` / ``df_maxunpool2x2``.  H and W must be multiples of 32
(480 x 640 is).

Training is opt-in: ``SegNet(trainable=True)`` (or ``net.trainable = True``).  The default module keeps its inference-only contract,
and its ``train()`` forward raises NotImplementedError.  A trainable module's ``train()`` forward runs the reference's graph on the
tape of segtrain_ops / train_ops: the UNFOLDED parameters (each
convolution with its bias on the fp32-MFMA kernel, weights arranged OHWI and padded like the eval path's), then BatchNorm2d with
batch statistics fused with the ReLU (and, at the encoder's stage ends, with the max-pool), writing the module's own
``running_mean`` / ``running_var`` / ``num_batches_tracked``.  It returns a [B,label_nbr,H,W] view of the channels-last logits; the
segmentation ``Loss`` (loss.py) reads the channels-last tensor behind it directly.  ``forward_nhwc`` of a trainable module in
``train()`` mode takes the channels-last [B,H,W,4] input ``df_seg_batch`` writes and returns the same.  ``label_nbr`` 2..64 trains: the
classifier's outputs are padded to a power of two and to 4 at the least.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, ops
from ..segtrain_ops import BatchNormReLU, BatchNormReLUMaxPool, MaxUnpool2x2
from ..train_ops import ConvAct

# (name, Cin, Cout) in forward order; 'P' = pool, 'U' = unpool (segnet.py:73-118)
_ENC = [("11", None, 64), ("12", 64, 64), "P", ("21", 64, 128), ("22", 128, 128), "P", ("31", 128, 256), ("32", 256, 256), ("33", 256, 256), "P",
        ("41", 256, 512), ("42", 512, 512), ("43", 512, 512), "P", ("51", 512, 512), ("52", 512, 512), ("53", 512, 512), "P"]
_DEC = ["U", ("53d", 512, 512), ("52d", 512, 512), ("51d", 512, 512), "U", ("43d", 512, 512), ("42d", 512, 512), ("41d", 512, 256),
        "U", ("33d", 256, 256), ("32d", 256, 256), ("31d", 256, 128), "U", ("22d", 128, 128), ("21d", 128, 64), "U", ("12d", 64, 64), ("11d", 64, None)]


def _pad4(n):
    return (n + 3) // 4 * 4


class SegNet(nn.Module):
    def __init__(self, input_nbr=3, label_nbr=22, trainable=False):
        super().__init__()
        self.input_nbr, self.label_nbr = input_nbr, label_nbr
        self.trainable = trainable             # plain attribute: not part of the state dict
        for item in _ENC + _DEC:
            if isinstance(item, str):
                continue
            name, cin, cout = item
            cin = input_nbr if cin is None else cin
            cout = label_nbr if cout is None else cout
            setattr(self, "conv" + name, nn.Conv2d(cin, cout, kernel_size=3, padding=1))
            if name != "11d":
                setattr(self, "bn" + name, nn.BatchNorm2d(cout, momentum=0.1))
        self._folded = {}          # name -> (version tag, w [Cout',3,3,Cin'] OHWI, b [Cout'])

    def _layer(self, name):
        conv = getattr(self, "conv" + name)
        bn = getattr(self, "bn" + name, None)
        tensors = [conv.weight, conv.bias] + ([bn.weight, bn.bias, bn.running_mean, bn.running_var] if bn is not None else [])
        tag = tuple((t.data_ptr(), t._version) for t in tensors)
        hit = self._folded.get(name)
        if hit is not None and hit[0] == tag:
            return hit[1], hit[2]
        with torch.no_grad():
            w, b = conv.weight.float(), conv.bias.float()
            if bn is not None:
                scale = bn.weight.float() / torch.sqrt(bn.running_var.float() + bn.eps)
                w = w * scale[:, None, None, None]
                b = (b - bn.running_mean.float()) * scale + bn.bias.float()
            cout, cin = w.shape[0], w.shape[1]
            w = w.permute(0, 2, 3, 1)                                     # OIHW -> OHWI
            w = F.pad(w, (0, _pad4(cin) - cin, 0, 0, 0, 0, 0, _pad4(cout) - cout)).contiguous()
            b = F.pad(b, (0, _pad4(cout) - cout)).contiguous()
        self._folded[name] = (tag, w, b)
        return w, b

    def fold(self):
        """Fold every BatchNorm into its convolution now, on the current stream (the eval forward otherwise folds a layer on its
        first use, on whatever stream that forward runs)."""
        for item in _ENC + _DEC:
            if not isinstance(item, str):
                self._layer(item[0])

    def _train_forward(self, x, taps=None):
        C = x.shape[1]
        a = x.detach().float().permute(0, 2, 3, 1)
        return self._train_forward_nhwc(F.pad(a, (0, _pad4(C) - C)).contiguous(), x.device, taps)

    def _train_forward_nhwc(self, a, device, taps=None):
        """The training graph on the channels-last, channel-padded input ``a`` (the tape's first tensor, not copied)."""
        self._folded = {}                     # the BatchNorm buffers are rewritten below, behind torch's version counters
        seq = _ENC + _DEC
        indices = []
        if taps is not None:
            taps["x"] = a
        with _lib.device_guard(device):
            for k, item in enumerate(seq):
                if item == "P":
                    continue                  # fused into the BatchNorm before it
                if item == "U":
                    a = MaxUnpool2x2.apply(a, indices.pop())
                    if taps is not None:
                        taps["u" + seq[k + 1][0]] = a
                    continue
                name = item[0]
                conv = getattr(self, "conv" + name)
                cout, cin = conv.weight.shape[0], conv.weight.shape[1]
                w = conv.weight.permute(0, 2, 3, 1)                                   # OIHW -> OHWI
                b = conv.bias
                # the classifier's outputs are padded to a power of two: its data gradient runs the flipped convolution, whose
                # input channels (these) the MFMA kernel takes in powers of two only (22 classes -> 32), and in fours at the least (2 or 3
                # classes -> 4)
                cpad = max(4, 1 << (cout - 1).bit_length()) if name == "11d" else _pad4(cout)
                if _pad4(cin) != cin or cpad != cout:
                    w = F.pad(w, (0, _pad4(cin) - cin, 0, 0, 0, 0, 0, cpad - cout))
                    b = F.pad(b, (0, cpad - cout))
                z = ConvAct.apply(a, w.contiguous(), b.contiguous(), None, None, 1, 1, 1, 0)
                if taps is not None:
                    taps["z" + name] = z
                bn = getattr(self, "bn" + name, None)
                if bn is None:
                    a = z
                    continue
                if bn.momentum is None or not bn.track_running_stats:
                    raise NotImplementedError("SegNet.train(): BatchNorm2d with momentum=None or without running statistics")
                args = (z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps)
                if k + 1 < len(seq) and seq[k + 1] == "P":
                    a, idx = BatchNormReLUMaxPool.apply(*args)
                    indices.append(idx)
                    if taps is not None:
                        taps["p" + name], taps["i" + name] = a, idx
                else:
                    a = BatchNormReLU.apply(*args)
                    if taps is not None:
                        taps["y" + name] = a
        out = a[..., :self.label_nbr].permute(0, 3, 1, 2)
        out._nhwc = a                         # Loss (loss.py) takes the channels-last logits from here
        return out

    def forward(self, x, taps=None):
        """``taps``: an optional dict that receives the intermediate tensors in forward order, channels-last and not copied (the
        tests' layer-by-layer view).  Keys: "x" the padded input; per layer NAME "zNAME" the convolution's output (training, and the
        classifier "z11d" in both modes), "yNAME" the BatchNorm + ReLU output (eval: of the folded convolution), "pNAME" / "iNAME"
        the pooled tensor and its uint8 index where a pool follows (training fuses the pool, so no "yNAME" there), "uNAME" the
        un-pooled input of decoder layer NAME.  In training they are the tape's own tensors."""
        if self.training and not self.trainable:
            raise NotImplementedError("SegNet: train() forward needs a module built with SegNet(trainable=True) (or net.trainable = True); "
                                      "the default module is inference-only")
        if not x.is_cuda:
            raise RuntimeError("densefusion_amd needs device tensors (no CPU path): call .cuda() on the input")
        B, C, H, W = x.shape
        if C != self.input_nbr or H % 32 or W % 32:
            raise RuntimeError(f"SegNet.forward: expected [B,{self.input_nbr},H,W] with H, W multiples of 32, got {tuple(x.shape)}")
        if self.training:
            return self._train_forward(x, taps)
        with torch.no_grad():
            a = x.detach().float().permute(0, 2, 3, 1)
            a = F.pad(a, (0, _pad4(C) - C)).contiguous()                  # NHWC, channels padded to 4
            return self.forward_nhwc(a, taps)[..., :self.label_nbr].permute(0, 3, 1, 2).contiguous()

    def forward_nhwc(self, x, taps=None):
        """Forward on the channels-last input x [B,H,W,pad4(input_nbr)] fp32 (padding channels zero; what df_segment_input and
        df_seg_batch write).  eval(): -> the channels-last activation [B,H,W,pad4(label_nbr)] whose first label_nbr channels are the
        logits.  train() (a trainable module only): x goes straight onto the tape, without the permute + pad copy of ``forward``, and
        the result is what ``forward`` returns in training: the [B,label_nbr,H,W] view with the channels-last logits attached.
        ``taps``: see ``forward``."""
        if self.training and not self.trainable:
            raise NotImplementedError("SegNet.forward_nhwc: train() needs a module built with SegNet(trainable=True); the default "
                                      "module is inference-only")
        if not x.is_cuda:
            raise RuntimeError("densefusion_amd needs device tensors (no CPU path): call .cuda() on the input")
        if x.dim() != 4 or x.shape[3] != _pad4(self.input_nbr) or x.shape[1] % 32 or x.shape[2] % 32 or x.dtype != torch.float32:
            raise RuntimeError(f"SegNet.forward_nhwc: expected fp32 [B,H,W,{_pad4(self.input_nbr)}] with H, W multiples of 32, "
                               f"got {tuple(x.shape)} {x.dtype}")
        if self.training:
            return self._train_forward_nhwc(x.detach().contiguous(), x.device, taps)
        L = _lib.lib()
        with torch.no_grad(), _lib.device_guard(x.device):
            a = x.contiguous()
            indices = []
            seq = _ENC + _DEC
            if taps is not None:
                taps["x"] = a
            for k, item in enumerate(seq):
                if item == "P":
                    b_, h, w_, c = a.shape
                    y = torch.empty(b_, h // 2, w_ // 2, c, device=a.device)
                    idx = torch.empty(b_, h // 2, w_ // 2, c, dtype=torch.uint8, device=a.device)
                    _lib.check(L.df_maxpool2x2_idx(a.data_ptr(), y.data_ptr(), idx.data_ptr(), b_, h, w_, c, _lib.current_stream()), "maxpool2x2_idx")
                    indices.append(idx)
                    a = y
                    if taps is not None:
                        taps["p" + seq[k - 1][0]], taps["i" + seq[k - 1][0]] = y, idx
                elif item == "U":
                    idx = indices.pop()
                    b_, h, w_, c = a.shape
                    y = torch.empty(b_, 2 * h, 2 * w_, c, device=a.device)
                    _lib.check(L.df_maxunpool2x2(a.data_ptr(), idx.data_ptr(), y.data_ptr(), b_, h, w_, c, _lib.current_stream()), "maxunpool2x2")
                    a = y
                    if taps is not None:
                        taps["u" + seq[k + 1][0]] = y
                else:
                    name = item[0]
                    w, b = self._layer(name)
                    act = 0 if name == "11d" else 1
                    if w.shape[3] >= 256:
                        a = ops.conv3x3_winograd_nhwc(a, w, b, dil=1, act=act)
                    else:
                        a = ops.conv2d_nhwc(a, w, b, stride=1, pad=1, dil=1, act=act)
                    if taps is not None:
                        taps[("y" if act else "z") + name] = a
            return a
