#!/usr/bin/env python3
"""Generate tests/golden/roi_sweep.npz: the REFERENCE's boxes and warp index maps on the seeded case family of tests/roi_common.py.

Runs only in the build container (needs the reference checkout, which never travels to the GPU box), like make_golden.py.
Every case's probability map is regenerated from its seed by tests/roi_common.py; the mask handed to the reference is the
kernels' contract on it, (1 - prob[..., 0] in float32) >= thr with NaN background, evaluated by torch.  Per geometry g:
  g<g>_geometry  (H, W, D, roi_size)
  g<g>_seed      [cases] the seed of each case (tests/roi_common.py case_seed), g<g>_classes / g<g>_thr its batch's C and threshold
  g<g>_box       [cases, 6] ROIBridge.get_mask_boundary2
  g<g>_fx, _fy   [cases, eval_h] / [cases, eval_w] get_transfer_index along H / W
  g<g>_bx, _by   [cases, H] / [cases, W] get_transfer_back_index along H / W
No masks and no feature tensors are stored.

    python tests/golden/make_golden_roi_sweep.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, '/root/reference')

from model import Unet_3Dblock as R_ub           # noqa: E402  (reference)

from tests import roi_common as RC               # noqa: E402


def main():
    out = {}
    n_cases = 0
    for g, (H, W, D, roi_size) in enumerate(RC.GEOMETRIES):
        torch.manual_seed(0)
        br = R_ub.ROIBridge(in_dim=8, d_model=32, nhead=1, dropout=0.3, N=1, roi_size=roi_size)
        geo = RC.roi_sizes(roi_size)
        assert (geo['eval_h'], geo['eval_w'], geo['min_h'], geo['min_w'], geo['h_roi'], geo['w_roi']) == \
            (br.eval_h_roi_size, br.eval_w_roi_size, br.min_h_roi, br.min_w_roi, br.h_roi_size, br.w_roi_size)
        n = len(RC.KINDS)
        rec = dict(box=np.zeros((n, 6), np.float32), fx=np.zeros((n, geo['eval_h']), np.float32), fy=np.zeros((n, geo['eval_w']), np.float32),
                   bx=np.zeros((n, H), np.float32), by=np.zeros((n, W), np.float32), seed=np.zeros(n, np.int64),
                   classes=np.zeros(n, np.int64), thr=np.zeros(n, np.float32))
        for gg, j, ks, C, thr in RC.batches():
            if gg != g:
                continue
            mask = RC.reference_mask(RC.make_batch(g, ks, C, thr), thr)
            box = br.get_mask_boundary2(mask.clone())
            x0, y0, _, x1, y1, _ = torch.split(box, 1, dim=1)
            fx = R_ub.get_transfer_index(x0, x1, H - 1, br.h_roi_size, br.eval_h_roi_size, device='cpu')
            fy = R_ub.get_transfer_index(y0, y1, W - 1, br.w_roi_size, br.eval_w_roi_size, device='cpu')
            bx = R_ub.get_transfer_back_index(x0, x1, H - 1, br.h_roi_size, br.eval_h_roi_size, 'cpu')
            by = R_ub.get_transfer_back_index(y0, y1, W - 1, br.w_roi_size, br.eval_w_roi_size, 'cpu')
            for b, k in enumerate(ks):
                rec['box'][k], rec['fx'][k], rec['fy'][k], rec['bx'][k], rec['by'][k] = box[b].numpy(), fx[b].numpy(), fy[b].numpy(), bx[b].numpy(), by[b].numpy()
                rec['seed'][k], rec['classes'][k], rec['thr'][k] = RC.case_seed(g, k), C, thr
                n_cases += 1
        out[f'g{g}_geometry'] = np.array((H, W, D, roi_size), np.int64)
        out.update({f'g{g}_{key}': v for key, v in rec.items()})
    path = os.path.join(HERE, 'roi_sweep.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes, {n_cases} cases, {len(out)} arrays)')


if __name__ == '__main__':
    main()
