"""DispNet (no cost volume) on the MI355X path: same names, attribute tree, state-dict keys and return
convention as models/dispnet.py.  The input of `conv1` is the concatenated pair; the two 5x5 stride-2 layers
that carry the most FLOPs of the encoder (conv2: 64 -> 128, conv3a: 128 -> 256) run on the MFMA kernel with a
5x5 window in eval mode when the `costvolume` option `conv2d_k5` is on, the seven 3x3 layers of 256 / 512 /
1024 channels (conv3b .. conv6b) on the wide MFMA kernel when `wide_conv2d` is on (csrc/conv_wide2d.hpp,
`util_conv.Conv2dReLU`) -- with both on, conv2 .. conv6b is one NHWC chain; each decoder level's bias + ReLU +
upsampling + myCat2d is one HIP launch in eval mode, and under autograd with the option `decoder_train`
(`costvolume.decoder_level`, csrc/decoder.hip); conv1 (7x7, 6 inputs), the iconv / deconv layers and the heads
are the reference's stock 2-D layers.  CPU tensors take the stock path in every layer."""
import torch
import torch.nn as nn

from .. import costvolume as cv
from .util_conv import conv2d_bn, deconv2d_bn, net_init

# (name, Cin, Cout, kernel, stride) of the encoder
_ENCODER = [("conv1", 6, 64, 7, 2), ("conv2", 64, 128, 5, 2), ("conv3a", 128, 256, 5, 2),
            ("conv3b", 256, 256, 3, 1), ("conv4a", 256, 512, 3, 2), ("conv4b", 512, 512, 3, 1),
            ("conv5a", 512, 512, 3, 2), ("conv5b", 512, 512, 3, 1), ("conv6a", 512, 1024, 3, 2),
            ("conv6b", 1024, 1024, 3, 1)]
# decoder level -> (deconv Cin, width, skip channels, the encoder layer whose output is the skip)
_DECODER = {5: (1024, 512, 512, "conv5b"), 4: (512, 256, 512, "conv4b"), 3: (256, 128, 256, "conv3b"),
            2: (128, 64, 128, "conv2"), 1: (64, 32, 64, "conv1")}


def _layer(fn, *a, **k):
    return fn(*a, flag_bias=True, bn=False, activefun=nn.ReLU(inplace=True), **k)


class dispnet(nn.Module):
    def __init__(self, maxdisparity=192):
        super(dispnet, self).__init__()
        self.name = "dispnet"
        self.D = maxdisparity
        self.delt = 1e-6
        self.count_levels = 7
        self.upsample = nn.Upsample(scale_factor=2, mode="bilinear")
        for name, cin, cout, k, s in _ENCODER:
            setattr(self, name, _layer(conv2d_bn, cin, cout, kernel_size=k, stride=s))
        self.pr6 = nn.Conv2d(1024, 1, kernel_size=3, stride=1, padding=1)
        for lvl in (5, 4, 3, 2, 1):
            cin, width, skip, _ = _DECODER[lvl]
            setattr(self, "deconv%d" % lvl, _layer(deconv2d_bn, cin, width, kernel_size=4, stride=2))
            setattr(self, "iconv%d" % lvl, _layer(conv2d_bn, width + 1 + skip, width,
                                                  kernel_size=3, stride=1))
            setattr(self, "pr%d" % lvl, nn.Conv2d(width, 1, kernel_size=3, stride=1, padding=1))
        net_init(self)
        for lvl in range(1, 7):                     # prediction heads start small (:61-62)
            head = getattr(self, "pr%d" % lvl)
            head.weight.data = head.weight.data * 0.1

    def forward(self, imL, imR, mode="train"):
        if imL.shape != imR.shape:
            raise ValueError("dispnet: imL and imR must have the same shape")   # :65
        maxD = max(self.D, imL.shape[-1])
        x = torch.cat([imL, imR], dim=1)
        skips = {}
        for name, _, _, _, _ in _ENCODER:
            x = getattr(self, name)(x)
            skips[name] = x
        # the MFMA layers hand NHWC maps from one to the next (util_conv.Conv2dReLU); the chain is left once
        x = x.contiguous()
        pr = self.pr6(x)
        out, out_scale = [pr], [6]
        for lvl in (5, 4, 3, 2, 1):
            # myCat2d(deconv(x), upsample(pr), skip): dispnet.py:89-90 and the levels below
            x = getattr(self, "iconv%d" % lvl)(
                cv.decoder_level(getattr(self, "deconv%d" % lvl), x, pr, skips[_DECODER[lvl][3]]))
            pr = getattr(self, "pr%d" % lvl)(x)
            out.insert(0, pr)
            out_scale.insert(0, lvl)
        out.insert(0, self.upsample(pr)[:, :, : imL.shape[-2], : imL.shape[-1]])
        out_scale.insert(0, 0)
        if mode == "test":
            out[-1] = out[-1].clamp(self.delt, maxD)   # the reference clamps out[-1] (:127)
        return out_scale, out
