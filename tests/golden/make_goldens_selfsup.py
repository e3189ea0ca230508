#!/usr/bin/env python3
"""Generate tests/golden/golden_selfsup.npz from the REFERENCE's self-supervised loss itself.

Runs only where the reference tree exists (never on the GPU box).  The reference's
``losses/SSIM.py`` and ``utils/imwrap.py`` are executed from their text as modules; the lines of
``losses/loss.py`` that the depthmono objective uses (:17-22 create_impyramid, :33-44 wfun and
diff1_dx/dy, :71-83 C_ds1, :196-236 loss_depthmono, :393-405 weight_common, :424-467
losses_pyramid1) are executed from the file text as methods of a holder class, the approach of
make_goldens.py (``ref_lines``) and oracle/reference_loader.py (``_exec_text``).  Shims, all
textual and applied to the lines read:
  1. Python-2 ``print`` statements (the ``flag_test`` blocks): dropped (flag_test is False);
  2. ``.data[0]`` on a 0-d tensor -> ``.item()`` (loss.py:202, 218-219, 402);
  3. the two uint8 mask lines in their PyTorch-0.3 meaning:
       loss.py:211  ((disp_wrap==0) + mask_ap).detach() > 1  ->  ((disp_wrap==0) & mask_ap).detach()
       loss.py:398  (disp_delt<3) - mask1                     ->  (disp_delt<3) & ~mask1
  4. ``Variable(`` -> ``(`` with its ``requires_grad=False`` keyword removed (loss.py:396).
Everything runs in float64 with torch's CPU generator seeded before the loss, so the reference's
own ``torch.rand(1)`` epsilon draws are reproducible: the product's losses_pyramid1, seeded the
same way, draws the same numbers in the same order.

The script REFUSES to write if the restatement (tests/selfsup_oracle.py) disagrees with the
reference by more than 1e-6 relative on the loss or on any gradient.

Usage:  python tests/golden/make_goldens_selfsup.py
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
from tests import selfsup_oracle as SO          # noqa: E402
from tests.golden.make_goldens import ref_lines  # noqa: E402

warnings.filterwarnings("ignore")


def load_reference():
    ssim_mod = RL._exec_text("SSIM", os.path.join(RL.REFERENCE_ROOT, "losses", "SSIM.py"))
    imwrap_mod = RL._exec_text("ref_imwrap", os.path.join(RL.REFERENCE_ROOT, "utils", "imwrap.py"))
    parts = [ref_lines("losses/loss.py", a, b) for a, b in
             ((33, 44), (71, 83), (196, 236), (393, 405), (424, 467))]
    body = []
    for part in parts:
        for l in part.splitlines():
            s = l.strip()
            if s.startswith("print ") or s.startswith("if(flag_test)") or s.startswith("if(flag_imshow"):
                continue                                                      # shim 1
            if "imsplot_tensor" in s or "matplotlib" in s or "plt." in s or s.startswith("dispLs[0], dispL1s[0]"):
                continue                                                      # the flag_imshow block
            l = l.replace(".data[0]", ".item()")                              # shim 2
            l = l.replace("((disp_wrap==0) + mask_ap).detach() > 1", "((disp_wrap==0) & mask_ap).detach()")
            l = l.replace("(disp_delt<3) - mask1", "(disp_delt<3) & ~mask1")  # shim 3
            l = l.replace("Variable(torch.zeros(disp_delt.shape), requires_grad=False)",
                          "(torch.zeros(disp_delt.shape))")                   # shim 4
            body.append("    " + l)
    create = ref_lines("losses/loss.py", 17, 22)
    ns = {"torch": torch, "F": F, "logging": __import__("logging"), "flag_test": False,
          "flag_imshow": False, "imwrap_BCHW": imwrap_mod.imwrap_BCHW}
    exec(create, ns)
    exec("class Ref(object):\n" + "\n".join(body) + "\n", ns)
    ref = ns["Ref"]()
    ref.w_ap, ref.w_ds, ref.w_lr = 1.0, 0.001, 0.001
    ref.ssim = ssim_mod.SSIM()
    ref.lossfun = ref.loss_depthmono
    return ref


def weight_levels(n, maxepoch, epoch):
    w = [0.01] * n
    x = (1 - epoch / float(maxepoch)) * (n - 1)
    idx = int(x)
    w[idx] = 1 - (x - idx)
    if idx < n - 1:
        w[idx + 1] = x - idx
    return w


def smooth(g, B, C, H, W, lo, hi, cell):
    coarse = torch.rand(B, C, max(2, H // cell + 2), max(2, W // cell + 2), generator=g, dtype=torch.float64)
    return lo + (hi - lo) * F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)


def rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def gen_case(ref, store, meta, case, B, H, W, nedge, n_levels, seed, epoch, maxepoch, dmax):
    g = torch.Generator().manual_seed(seed)
    batch_u8 = (smooth(g, B, 6, H, W, 0, 255, 6) + 12 * torch.rand(B, 6, H, W, generator=g, dtype=torch.float64))
    batch_u8 = batch_u8.clamp(0, 255).round().to(torch.uint8)
    batch = batch_u8.double() / 255.0
    h, w = H - 2 * nedge, W - 2 * nedge
    dLs = [smooth(g, B, 1, -(-h // 2 ** k), -(-w // 2 ** k), 0.5, dmax, 4).float() / 2 ** k for k in range(n_levels)]
    dL1s = [smooth(g, B, 1, -(-h // 2 ** k), -(-w // 2 ** k), 0.5, dmax, 4).float() / 2 ** k for k in range(n_levels)]
    store[case + ".batch"] = batch_u8.numpy()
    for i in range(n_levels):
        store["%s.dispL.%d" % (case, i)] = dLs[i].numpy()
        store["%s.dispL1.%d" % (case, i)] = dL1s[i].numpy()
    wl = weight_levels(n_levels, maxepoch, epoch)
    batch1 = torch.flip(batch, dims=[-1])
    names = ["depthmono", "depthmono-mask"]
    for name in names:
        flag_mask = "mask" in name
        ref.flag_mask, ref.weight_levels = flag_mask, wl
        ins = [d.double().requires_grad_() for d in dLs + dL1s]
        args = {"imR_src": batch[:, 3:6], "imL": batch[:, :3, nedge:H - nedge, nedge:W - nedge],
                "dispLs": ins[:n_levels], "scale_dispLs": list(range(n_levels)), "LeftTop": [nedge, nedge],
                "imR1_src": batch1[:, :3], "imL1": batch1[:, 3:6, nedge:H - nedge, nedge:W - nedge],
                "dispL1s": ins[n_levels:], "scale_dispL1s": list(range(n_levels)), "LeftTop1": [nedge, nedge]}
        torch.manual_seed(seed)
        want = ref.losses_pyramid1(**args)
        want.backward()
        mine_in = [d.double().requires_grad_() for d in dLs + dL1s]
        torch.manual_seed(seed)
        mine, _ = SO.losses_pyramid1(wl, flag_mask, args["imR_src"], args["imL"], mine_in[:n_levels],
                                     args["scale_dispLs"], args["LeftTop"], args["imR1_src"], args["imL1"],
                                     mine_in[n_levels:], args["LeftTop1"])
        mine.backward()
        tag = "%s.%s" % (case, name)
        e_loss = rel(mine.detach(), want.detach())
        e_grad = max(rel(a.grad, b.grad) for a, b in zip(mine_in, ins))
        print("  %-28s loss %.8f  rel(loss) %.2e  max rel(grad) %.2e" % (tag, float(want), e_loss, e_grad))
        if e_loss > 1e-6 or e_grad > 1e-6:
            raise SystemExit("restatement disagrees with the reference on %s" % tag)
        store[tag + ".loss"] = np.float64(float(want))
        for i in range(n_levels):
            store["%s.gL.%d" % (tag, i)] = ins[i].grad.float().numpy()
            store["%s.gL1.%d" % (tag, i)] = ins[n_levels + i].grad.float().numpy()
    meta["cases"][case] = {"names": names, "seed": seed, "nedge": nedge, "levels": n_levels, "B": B,
                           "H": H, "W": W, "count_levels": n_levels, "maxepoch": maxepoch, "epoch": epoch}


def main():
    if not RL.available():
        raise SystemExit("needs the reference tree at %s" % RL.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    ref = load_reference()
    store, meta = {}, {"torch": torch.__version__, "align_corners": False, "cases": {},
                       "reference": "sunshinnnn/DSMnet losses/loss.py, losses/SSIM.py, utils/imwrap.py"}
    print("selfsup goldens (float64, reference lines executed from the file text)")
    # dispnetcorr-shaped: 7 outputs, nedge 64 (the -mask preset), 64x128 loss crop
    gen_case(ref, store, meta, "pyr7", 1, 192, 256, 64, 7, 101, 3, 10, 16.0)
    # small ragged case: 4 outputs on 37x101, no crop
    gen_case(ref, store, meta, "ragged", 2, 37, 101, 0, 4, 202, 1, 4, 10.0)
    store["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "golden_selfsup.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%.1f KiB, %d arrays)" % (path, os.path.getsize(path) / 1024.0, len(store)))


if __name__ == "__main__":
    main()
