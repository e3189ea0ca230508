#!/usr/bin/env python3
"""Generate tests/golden/golden_sssmnet.npz from the REFERENCE's "SsSMnet[-mask]" and
"common[-mask]" losses themselves.

Runs only where the reference tree exists (never on the GPU box).  As make_goldens_cap.py does:
``losses/SSIM.py`` and ``utils/imwrap.py`` are executed from their text as modules, and the lines
of ``losses/loss.py`` that the objectives use (:17-22 create_impyramid, :33-44 wfun and
diff1_dx/dy, :46-54 diff2_dx/dy, :56-64 diff_z_dx/dy, :66-69 C_imdiff1, :85-114 C_ds2 and C_ds3,
:154-194 loss_common, :285-324 loss_SsSMnet, :393-405 weight_common, :424-467 losses_pyramid1,
:469-512 losses_pyramid2) are executed from the file text as methods of a holder class.  The
textual shims are that generator's four: the Python-2 ``print`` lines dropped, ``.data[0]`` ->
``.item()``, the uint8 mask lines in their PyTorch-0.3 meaning (loss.py:171, 300, 398; DESIGN.md
section 12) and ``Variable(`` unwrapped.

Everything runs in float64 with torch's CPU generator seeded before the loss, so the reference's
own ``torch.rand(1)`` epsilon draws are reproducible; the draw that follows the loss is recorded
and compared with the restatement's (the draw count and order: four per weighted entry, six for
SsSMnet-mask).  The value of ``wfun`` is recorded for every view.

The script REFUSES to write if the restatement (tests/sssmnet_oracle.py) disagrees with the
reference by more than 1e-6 relative on the loss or on any gradient.

Usage:  python tests/golden/make_goldens_sssmnet.py
"""
import json
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import reference_loader as RL       # noqa: E402
from tests import sssmnet_oracle as XO          # noqa: E402
from tests.golden.make_goldens import ref_lines  # noqa: E402
from tests.golden.make_goldens_selfsup import rel, smooth, weight_levels  # noqa: E402

warnings.filterwarnings("ignore")


def load_reference():
    ssim_mod = RL._exec_text("SSIM", os.path.join(RL.REFERENCE_ROOT, "losses", "SSIM.py"))
    imwrap_mod = RL._exec_text("ref_imwrap", os.path.join(RL.REFERENCE_ROOT, "utils", "imwrap.py"))
    parts = [ref_lines("losses/loss.py", a, b) for a, b in
             ((33, 44), (46, 54), (56, 64), (66, 69), (85, 114), (154, 194), (285, 324), (393, 405),
              (424, 467), (469, 512))]
    body = []
    for part in parts:
        for l in part.splitlines():
            s = l.strip()
            if s.startswith("print ") or s.startswith("if(flag_test)") or s.startswith("if(flag_imshow"):
                continue
            if ("imsplot_tensor" in s or "matplotlib" in s or "plt." in s or s.startswith("dispLs[0], dispL1s[0]")):
                continue
            l = l.replace(".data[0]", ".item()")
            l = l.replace("((disp_wrap==0) + mask_ap).detach() > 1", "((disp_wrap==0) & mask_ap).detach()")
            l = l.replace("((im_wrap1[:, :1] == 0) + mask_ap).detach() > 1", "((im_wrap1[:, :1] == 0) & mask_ap).detach()")
            l = l.replace("(disp_delt<3) - mask1", "(disp_delt<3) & ~mask1")
            l = l.replace("Variable(torch.zeros(disp_delt.shape), requires_grad=False)",
                          "(torch.zeros(disp_delt.shape))")
            body.append("    " + l)
    create = ref_lines("losses/loss.py", 17, 22)
    ns = {"torch": torch, "F": F, "logging": __import__("logging"), "flag_test": False,
          "flag_imshow": False, "imwrap_BCHW": imwrap_mod.imwrap_BCHW}
    exec(create, ns)
    exec("class Ref(object):\n" + "\n".join(body) + "\n", ns)
    ref = ns["Ref"]()
    ref.w_ap, ref.w_ds, ref.w_lr, ref.w_m = 1.0, 0.001, 0.001, 0.0001      # loss.py:27-30
    ref.ssim = ssim_mod.SSIM()
    return ref


def set_name(ref, name, wl):
    """losses.__init__ and setlossfun (loss.py:345-346, 362-377) for the two families."""
    ref.flag_mask = "mask" in name
    ref.loss_name = name.split("-")[0].lower()
    ref.weight_levels = wl
    if "sssmnet" in ref.loss_name:
        ref.lossfun, ref.lossesfun = ref.loss_SsSMnet, ref.losses_pyramid2
        return "sssmnet"
    ref.lossfun, ref.lossesfun = ref.loss_common, ref.losses_pyramid1
    return "common"


def gen_case(ref, store, meta, case, names, B, H, W, nedge, n_levels, seed, epoch, maxepoch, dlo, dhi,
             contrast=1.0, w_above_floor=()):
    g = torch.Generator().manual_seed(seed)
    batch_u8 = (smooth(g, B, 6, H, W, 0, 255, 6) + 12 * torch.rand(B, 6, H, W, generator=g, dtype=torch.float64))
    batch_u8 = (127.5 + contrast * (batch_u8 - 127.5)).clamp(0, 255).round().to(torch.uint8)
    batch = batch_u8.double() / 255.0
    h, w = H - 2 * nedge, W - 2 * nedge

    def disp(k):
        # per-pixel noise on the smooth field: a bilinear field alone has second differences of
        # rounding size, and the sign of such a |diff2| is no property of the objective
        hk, wk = -(-h // 2 ** k), -(-w // 2 ** k)
        return ((smooth(g, B, 1, hk, wk, dlo, dhi, 4) + 0.3 * torch.rand(B, 1, hk, wk, generator=g, dtype=torch.float64))
                .float() / 2 ** k)
    dLs = [disp(k) for k in range(n_levels)]
    dL1s = [disp(k) for k in range(n_levels)]
    store[case + ".batch"] = batch_u8.numpy()
    for i in range(n_levels):
        store["%s.dispL.%d" % (case, i)] = dLs[i].numpy()
        store["%s.dispL1.%d" % (case, i)] = dL1s[i].numpy()
    wl = weight_levels(n_levels, maxepoch, epoch)
    batch1 = torch.flip(batch, dims=[-1])
    for name in names:
        objective = set_name(ref, name, wl)
        ws, wfun = [], type(ref).wfun

        def recording(similarity, ws=ws, wfun=wfun):
            ws.append(wfun(ref, similarity))
            return ws[-1]
        ref.wfun = recording
        ins = [d.double().requires_grad_() for d in dLs + dL1s]
        args = {"imR_src": batch[:, 3:6], "imL": batch[:, :3, nedge:H - nedge, nedge:W - nedge],
                "dispLs": ins[:n_levels], "scale_dispLs": list(range(n_levels)), "LeftTop": [nedge, nedge],
                "imR1_src": batch1[:, :3], "imL1": batch1[:, 3:6, nedge:H - nedge, nedge:W - nedge],
                "dispL1s": ins[n_levels:], "scale_dispL1s": list(range(n_levels)), "LeftTop1": [nedge, nedge]}
        torch.manual_seed(seed)
        want = ref.lossesfun(**args)
        next_ref = float(torch.rand(1)[0])           # the draw that follows the reference's own
        want.backward()
        del ref.wfun
        mine_in = [d.double().requires_grad_() for d in dLs + dL1s]
        stats = []
        torch.manual_seed(seed)
        mine, used = XO.losses_pyramid(objective, wl, ref.flag_mask, args["imR_src"], args["imL"],
                                       mine_in[:n_levels], args["scale_dispLs"], args["LeftTop"],
                                       args["imR1_src"], args["imL1"], mine_in[n_levels:], args["LeftTop1"],
                                       stats=stats)
        if float(torch.rand(1)[0]) != next_ref:
            raise SystemExit("%s %s: the restatement left the CPU generator in another state" % (case, name))
        mine.backward()
        tag = "%s.%s" % (case, name)
        e_loss = rel(mine.detach(), want.detach())
        e_grad = max(rel(a.grad, b.grad) for a, b in zip(mine_in, ins))
        e_w = max(abs(float(s[0]) - v) / v for s, v in zip(stats, ws))
        second = [int(s[1]) for s in stats]          # common: the fallback flag; SsSMnet: valid pixels
        print("  %-26s loss %.8f  rel(loss) %.2e  max rel(grad) %.2e  rel(w) %.2e  w %s  %s %s" % (
            tag, float(want), e_loss, e_grad, e_w, ["%.4f" % v for v in ws],
            "fallback" if objective == "common" else "valid", second))
        if not (e_loss <= 1e-6 and e_grad <= 1e-6 and e_w <= 1e-6) or len(ws) != len(stats):
            raise SystemExit("restatement disagrees with the reference on %s" % tag)
        if name in w_above_floor and not min(ws) > 0.002:
            raise SystemExit("%s: meant to have w above its floor, has w %s" % (tag, ws))
        store[tag + ".loss"] = np.float64(float(want))
        store[tag + ".w"] = np.array(ws, dtype=np.float64)          # per weighted entry: left view, flipped view
        store[tag + ".second"] = np.array(second, dtype=np.int64)
        store[tag + ".next"] = np.float64(next_ref)                 # where the CPU generator stands after the loss
        store[tag + ".draws"] = np.int64(sum(len(u) for u in used))
        for i in range(n_levels):
            store["%s.gL.%d" % (tag, i)] = ins[i].grad.numpy()
            store["%s.gL1.%d" % (tag, i)] = ins[n_levels + i].grad.numpy()
    meta["cases"][case] = {"names": names, "seed": seed, "nedge": nedge, "levels": n_levels, "B": B,
                           "H": H, "W": W, "count_levels": n_levels, "maxepoch": maxepoch, "epoch": epoch}


ALL = ["SsSMnet", "SsSMnet-mask", "common", "common-mask"]


def main():
    if not RL.available():
        raise SystemExit("needs the reference tree at %s" % RL.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    ref = load_reference()
    store, meta = {}, {"torch": torch.__version__, "align_corners": False, "cases": {},
                       "reference": "sunshinnnn/DSMnet losses/loss.py, losses/SSIM.py, utils/imwrap.py"}
    print("SsSMnet / common goldens (float64, reference lines executed from the file text)")
    # dispnetcorr-shaped (scale_dispLs 0..6), nedge 16, 32x96 loss crop; epoch 3 of 10: levels 4 and
    # 5 carry 0.8 and 0.2, the others 0.01 -- levels 3..6 are upsampled to the level-2 grid
    gen_case(ref, store, meta, "pyr7", ALL, 1, 64, 128, 16, 7, 401, 3, 10, 0.5, 16.0)
    # low-contrast images, a fifth of the samples outside, 2560 pixels per view (no fallback): the
    # masked mean SSIM is above 0.75, so w is above its floor of 0.001 under both rules
    gen_case(ref, store, meta, "lowcontrast", ALL, 1, 40, 64, 0, 1, 404, 0, 1, 4.0, 12.0, contrast=0.02,
             w_above_floor=ALL)
    # every disparity beyond the source width: mask_ap selects nothing (SsSMnet: w = 0.001; common:
    # fewer than 1024 valid, every pixel counts)
    gen_case(ref, store, meta, "novalid", ALL, 1, 24, 40, 0, 1, 403, 0, 1, 50.0, 60.0)
    # 960 pixels per view, a third of the samples outside: common's "< 1024 valid" fallback
    gen_case(ref, store, meta, "sub1024", ALL, 1, 24, 40, 0, 1, 402, 0, 1, 0.5, 30.0)
    store["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "golden_sssmnet.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%.1f KiB, %d arrays)" % (path, os.path.getsize(path) / 1024.0, len(store)))


if __name__ == "__main__":
    main()
