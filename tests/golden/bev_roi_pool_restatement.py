"""SECONDHead.roi_grid_pool restated in numpy, float64 by default: what torch computes for the reference's code
(second_head.py:53-110) with align_corners=False in affine_grid and grid_sample, bilinear, zero padding -- the statement of
pda_bev_roi_grid_pool in include/pda_train.h, written independently of csrc/bev_roi_grid.h."""
import numpy as np


def positions(rois, g, h, w, min_x, min_y, cell_x, cell_y, dtype=np.float64):
    """rois (..., 7) -> ix, iy (..., g, g): the sampling position of grid row i, column j on the (h, w) map."""
    r = np.asarray(rois).astype(dtype)
    T = dtype
    with np.errstate(all='ignore'):
        x1 = (r[..., 0] - r[..., 3] / T(2) - T(min_x)) / T(cell_x)
        x2 = (r[..., 0] + r[..., 3] / T(2) - T(min_x)) / T(cell_x)
        y1 = (r[..., 1] - r[..., 4] / T(2) - T(min_y)) / T(cell_y)
        y2 = (r[..., 1] + r[..., 4] / T(2) - T(min_y)) / T(cell_y)
        cosa, sina = np.cos(r[..., 6]), np.sin(r[..., 6])
        t0, t1, t2 = (x2 - x1) / T(w - 1) * cosa, (x2 - x1) / T(w - 1) * (-sina), (x1 + x2 - T(w) + T(1)) / T(w - 1)
        t3, t4, t5 = (y2 - y1) / T(h - 1) * sina, (y2 - y1) / T(h - 1) * cosa, (y1 + y2 - T(h) + T(1)) / T(h - 1)
        k = np.arange(g).astype(dtype)
        lin = (T(2) * k + T(1)) / T(g) - T(1)
        u, v = lin[None, :], lin[:, None]                                  # column j, row i
        e = lambda t: t[..., None, None]
        gx = e(t0) * u + e(t1) * v + e(t2)
        gy = e(t3) * u + e(t4) * v + e(t5)
        ix = ((gx + T(1)) * T(w) - T(1)) / T(2)
        iy = ((gy + T(1)) * T(h) - T(1)) / T(2)
    return ix, iy


def roi_grid_pool(bev, rois, g, min_x, min_y, cell_x, cell_y, dtype=np.float64):
    """bev (B, C, H, W), rois (B, R, 7) -> (B * R, C, g, g) in `dtype`.  A position that is not finite or lies outside
    [-1, w) x [-1, h) gives 0."""
    bev = np.asarray(bev).astype(dtype)
    B, C, H, W = bev.shape
    R = rois.shape[1]
    ix, iy = positions(rois, g, H, W, min_x, min_y, cell_x, cell_y, dtype)                      # (B, R, g, g)
    with np.errstate(all='ignore'):
        live = np.isfinite(ix) & np.isfinite(iy) & (ix >= -1) & (ix < W) & (iy >= -1) & (iy < H)
    ix, iy = np.where(live, ix, 0), np.where(live, iy, 0)
    x0, y0 = np.floor(ix), np.floor(iy)
    out = np.zeros((B, R, C, g, g), dtype)
    scene = np.arange(B)[:, None, None, None]
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):                                            # nw, ne, sw, se
        wx = (ix - x0) if dx else (x0 + 1 - ix)
        wy = (iy - y0) if dy else (y0 + 1 - iy)
        xi, yi = x0.astype(np.int64) + dx, y0.astype(np.int64) + dy
        inside = live & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        vals = bev[scene, :, np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]                     # (B, R, g, g, C)
        out += np.moveaxis(np.where(inside[..., None], vals * (wx * wy)[..., None], 0), -1, 2)
    return out.reshape(B * R, C, g, g)


def classify(rois, g, h, w, min_x, min_y, cell_x, cell_y):
    """Per RoI (B, R): 'inside' (no sample touches the zero padding), 'outside' (no sample reads the map), or a string of the
    borders that cut it out of 'l', 'r', 't', 'b' (x below 0, x above w - 1, y below 0, y above h - 1)."""
    ix, iy = positions(rois, g, h, w, min_x, min_y, cell_x, cell_y)
    B, R = ix.shape[:2]
    res = np.empty((B, R), dtype=object)
    for b in range(B):
        for r in range(R):
            x, y = ix[b, r], iy[b, r]
            reads = (x > -1) & (x < w) & (y > -1) & (y < h)
            if not reads.any():
                res[b, r] = 'outside'
                continue
            cut = ('l' if (x < 0).any() else '') + ('r' if (x > w - 1).any() else '') + ('t' if (y < 0).any() else '') \
                + ('b' if (y > h - 1).any() else '')
            res[b, r] = cut or 'inside'
    return res
