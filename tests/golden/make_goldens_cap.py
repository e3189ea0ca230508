#!/usr/bin/env python3
"""Generate tests/golden/golden_cap.npz from the REFERENCE's "Cap[_ds][_lr][-mask]" loss itself.

Runs only where the reference tree exists (never on the GPU box).  As make_goldens_selfsup.py
does: ``losses/SSIM.py`` and ``utils/imwrap.py`` are executed from their text as modules, and the
lines of ``losses/loss.py`` that the objective uses (:17-22 create_impyramid, :33-44 wfun and
diff1_dx/dy, :71-83 C_ds1, :238-283 loss_Cap_ds_lr, :393-405 weight_common, :424-467
losses_pyramid1) are executed from the file text as methods of a holder class (``ref_lines`` of
make_goldens.py, ``_exec_text`` of oracle/reference_loader.py).  The textual shims are that
generator's four: the Python-2 ``print`` lines dropped, ``.data[0]`` -> ``.item()``, the two
uint8 mask lines in their PyTorch-0.3 meaning (loss.py:253, 398) and
``Variable(`` unwrapped.  ``self.loss_name`` is what losses.__init__ makes of the name
(loss.py:345-346: the part before "-", lower-cased), ``flag_mask`` is ``"mask" in name``.

Everything runs in float64 with torch's CPU generator seeded before the loss, so the reference's
own ``torch.rand(1)`` epsilon draws are reproducible.  Gradients are stored in float64 (the CPU test
holds the restatement to 1e-12).  The value of ``wfun`` is recorded for every
view (the "novalid" case pins what the reference gives when mask_ap selects nothing).

The script REFUSES to write if the restatement (tests/cap_oracle.py) disagrees with the
reference by more than 1e-6 relative on the loss or on any gradient.

Usage:  python tests/golden/make_goldens_cap.py
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
from tests import cap_oracle as CO              # noqa: E402
from tests.golden.make_goldens import ref_lines  # noqa: E402
from tests.golden.make_goldens_selfsup import rel, smooth, weight_levels  # noqa: E402

warnings.filterwarnings("ignore")


def load_reference():
    ssim_mod = RL._exec_text("SSIM", os.path.join(RL.REFERENCE_ROOT, "losses", "SSIM.py"))
    imwrap_mod = RL._exec_text("ref_imwrap", os.path.join(RL.REFERENCE_ROOT, "utils", "imwrap.py"))
    parts = [ref_lines("losses/loss.py", a, b) for a, b in
             ((33, 44), (71, 83), (238, 283), (393, 405), (424, 467))]
    body = []
    for part in parts:
        for l in part.splitlines():
            s = l.strip()
            if s.startswith("print ") or s.startswith("if(flag_test)") or s.startswith("if(flag_imshow"):
                continue
            if "imsplot_tensor" in s or "matplotlib" in s or "plt." in s or s.startswith("dispLs[0], dispL1s[0]"):
                continue
            l = l.replace(".data[0]", ".item()")
            l = l.replace("((disp_wrap==0) + mask_ap).detach() > 1", "((disp_wrap==0) & mask_ap).detach()")
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
    ref.w_ap, ref.w_ds, ref.w_lr = 1.0, 0.001, 0.001
    ref.ssim = ssim_mod.SSIM()
    ref.lossfun = ref.loss_Cap_ds_lr
    return ref


def set_name(ref, name, wl):
    ref.flag_mask = "mask" in name                       # loss.py:345
    ref.loss_name = name.split("-")[0].lower()           # loss.py:346, 351
    ref.weight_levels = wl


def gen_case(ref, store, meta, case, names, B, H, W, nedge, n_levels, seed, epoch, maxepoch, dlo, dhi,
             contrast=1.0, need_w_above_floor=False):
    g = torch.Generator().manual_seed(seed)
    batch_u8 = (smooth(g, B, 6, H, W, 0, 255, 6) + 12 * torch.rand(B, 6, H, W, generator=g, dtype=torch.float64))
    batch_u8 = (127.5 + contrast * (batch_u8 - 127.5)).clamp(0, 255).round().to(torch.uint8)
    batch = batch_u8.double() / 255.0
    h, w = H - 2 * nedge, W - 2 * nedge
    dLs = [smooth(g, B, 1, -(-h // 2 ** k), -(-w // 2 ** k), dlo, dhi, 4).float() / 2 ** k for k in range(n_levels)]
    dL1s = [smooth(g, B, 1, -(-h // 2 ** k), -(-w // 2 ** k), dlo, dhi, 4).float() / 2 ** k for k in range(n_levels)]
    store[case + ".batch"] = batch_u8.numpy()
    for i in range(n_levels):
        store["%s.dispL.%d" % (case, i)] = dLs[i].numpy()
        store["%s.dispL1.%d" % (case, i)] = dL1s[i].numpy()
    wl = weight_levels(n_levels, maxepoch, epoch)
    batch1 = torch.flip(batch, dims=[-1])
    for name in names:
        set_name(ref, name, wl)
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
        want = ref.losses_pyramid1(**args)
        want.backward()
        del ref.wfun
        mine_in = [d.double().requires_grad_() for d in dLs + dL1s]
        stats = []
        torch.manual_seed(seed)
        mine, _ = CO.losses_pyramid1(wl, ref.flag_mask, CO.terms_of(name), args["imR_src"], args["imL"],
                                     mine_in[:n_levels], args["scale_dispLs"], args["LeftTop"],
                                     args["imR1_src"], args["imL1"], mine_in[n_levels:], args["LeftTop1"],
                                     stats=stats)
        mine.backward()
        tag = "%s.%s" % (case, name)
        e_loss = rel(mine.detach(), want.detach())
        e_grad = max(rel(a.grad, b.grad) for a, b in zip(mine_in, ins))
        e_w = max(abs(float(s[0]) - v) / v for s, v in zip(stats, ws))
        print("  %-28s loss %.8f  rel(loss) %.2e  max rel(grad) %.2e  rel(w) %.2e  valid %s" % (
            tag, float(want), e_loss, e_grad, e_w, [int(s[1]) for s in stats]))
        if not (e_loss <= 1e-6 and e_grad <= 1e-6 and e_w <= 1e-6) or len(ws) != len(stats):
            raise SystemExit("restatement disagrees with the reference on %s" % tag)
        if need_w_above_floor and not (min(ws) > 0.002 and all(0 < int(s[1]) < 0.9 * B * h * w for s in stats)):
            raise SystemExit("%s: meant to have w above its floor and invalid pixels, has w %s" % (tag, ws))
        store[tag + ".loss"] = np.float64(float(want))
        store[tag + ".w"] = np.array(ws, dtype=np.float64)          # per weighted entry: left view, flipped view
        store[tag + ".valid"] = np.array([int(s[1]) for s in stats], dtype=np.int64)
        for i in range(n_levels):
            store["%s.gL.%d" % (tag, i)] = ins[i].grad.numpy()
            store["%s.gL1.%d" % (tag, i)] = ins[n_levels + i].grad.numpy()
    meta["cases"][case] = {"names": names, "seed": seed, "nedge": nedge, "levels": n_levels, "B": B,
                           "H": H, "W": W, "count_levels": n_levels, "maxepoch": maxepoch, "epoch": epoch}


def main():
    if not RL.available():
        raise SystemExit("needs the reference tree at %s" % RL.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    ref = load_reference()
    store, meta = {}, {"torch": torch.__version__, "align_corners": False, "cases": {},
                       "reference": "sunshinnnn/DSMnet losses/loss.py, losses/SSIM.py, utils/imwrap.py"}
    print("Cap goldens (float64, reference lines executed from the file text)")
    # dispnetcorr-shaped (scale_dispLs 0..6), nedge 64, 32x128 loss crop; epoch 3 of 10: levels 4
    # and 5 carry 0.8 and 0.2, the others 0.01 -- the divisors 8..64 against scale_factor 4
    gen_case(ref, store, meta, "pyr7", ["Cap_ds-mask", "Cap_ds"], 1, 160, 256, 64, 7, 301, 3, 10, 0.5, 16.0)
    # no smoothness term; and the left-right term, which only the op takes
    gen_case(ref, store, meta, "small", ["Cap-mask", "Cap_ds_lr-mask"], 2, 36, 56, 0, 3, 302, 1, 4, 0.5, 10.0)
    # low-contrast images, a fifth of the samples outside: the masked mean SSIM is above 0.75 while
    # the mean over every pixel is not, so w is above its floor of 0.001 and is the masked mean's --
    # the one case in which the restatement's simlary and w are held to the reference's own lines
    gen_case(ref, store, meta, "lowcontrast", ["Cap_ds-mask"], 1, 24, 40, 0, 1, 304, 0, 1, 4.0, 12.0,
             contrast=0.02, need_w_above_floor=True)
    # every disparity beyond the source width: mask_ap selects nothing
    gen_case(ref, store, meta, "novalid", ["Cap_ds-mask"], 1, 24, 40, 0, 1, 303, 0, 1, 50.0, 60.0)
    store["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "golden_cap.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%.1f KiB, %d arrays)" % (path, os.path.getsize(path) / 1024.0, len(store)))


if __name__ == "__main__":
    main()
