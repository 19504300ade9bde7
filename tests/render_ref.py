"""Yardstick of the depth renderer: a restatement of the reference's RegistrationRender (models/render.py:27-73) with a dtype
argument, the argmax of every pixel, and the analytic backward of include/scream_hip.h (optionally under a given argmax map, so
a gradient can be checked under the kernel's own choice of point).  Runs on whatever device the inputs are on."""
import numpy as np
import torch

from scream_amd.render import rotation_matrix, view_eulers


def pixel_centres(w: int, dtype=torch.float32, device="cpu") -> torch.Tensor:
    """render.py:14-16: [w*w, 2] (x = column, y = row)."""
    i, j = np.arange(w * w) // w, np.arange(w * w) % w
    pix = torch.from_numpy(np.concatenate([j.reshape(-1, 1), i.reshape(-1, 1)], axis=1)).to(dtype).to(device)
    return (pix - w // 2 + 0.5) / (w // 2)


def _rotate(R, pts, dtype):
    return torch.matmul(R.to(device=pts.device, dtype=dtype), pts.T).T


def split_plan(w: int, n_pairs: int, n_views: int, max_len: int):
    """(splits, per_split) of the splat launch: a line-for-line restatement of the rule in scream_render_depth
    (csrc/render.hip), with its constants TILE = 32, SUB = 256 and its target of 2 048 blocks.  A splat block scans its
    staging buffer in the middle of its range only when more than CAP - SUB = 768 of its per_split points are staged, so a
    test that claims that path asserts on per_split first.  max_len > 0."""
    tiles = (w // 32) * (w // 32)
    n_range = n_pairs * n_views * 2
    base = tiles * n_range
    splits = (2048 + base - 1) // base
    max_splits = (max_len + 256 - 1) // 256
    splits = splits if splits < max_splits else max_splits
    splits = 1 if splits < 1 else splits
    per_split = (max_len + splits - 1) // splits
    splits = (max_len + per_split - 1) // per_split
    return splits, per_split


POINT_CHUNK = 4096  # points per [points, 4096 pixels, 2] block of render(): 268 MB in float64


def render(src_pred, tgt, rho=24, w=64, eulers=None, dtype=torch.float32, top2=False):
    """Returns (imgs [V,2,w,w], argmax [V,2,w,w] int64, ranges [(dmin, dmax)] per view[, gap [V,2,w,w]: top-1 minus top-2 value]).
    In fp32 the images are the reference's bit for bit (same operations in the same order on every element; a side's points
    are taken POINT_CHUNK at a time, which changes no value: the maximum is exact, the lower chunk keeps a tie)."""
    eulers = view_eulers("muti") if eulers is None else eulers
    n = src_pred.shape[0]
    x = torch.cat([src_pred, tgt], dim=0).to(dtype)
    pix_xy = pixel_centres(w, dtype, x.device)
    imgs, amax, ranges, gaps = [], [], [], []
    for e in eulers:
        X = _rotate(rotation_matrix(e), x, dtype)
        depth = X[:, 2]
        dmin, dmax = torch.min(depth, dim=0)[0].item(), torch.max(depth, dim=0)[0].item()
        pv = 1 - (depth - dmin) / (dmax - dmin)
        ranges.append((dmin, dmax))
        bw2 = 64 * 64
        out = [[], []]
        idx = [[], []]
        gap = [[], []]
        for c in range((w // 64) ** 2):
            s0, s1 = c * bw2, (c + 1) * bw2
            for side, (k_lo, k_hi) in ((0, (0, n)), (1, (n, x.shape[0]))):
                mv = mi = second = None
                for k0 in range(k_lo, k_hi, POINT_CHUNK):
                    k1 = min(k_hi, k0 + POINT_CHUNK)
                    pw = ((X[k0:k1, :2].view(-1, 1, 2).repeat([1, bw2, 1]) - pix_xy[s0:s1].unsqueeze(0)) ** 2).sum(dim=2)
                    pw = torch.exp(-pw / 2 * rho ** 2)
                    val = pv.view(-1, 1)[k0:k1] * pw
                    cv, ci = torch.max(val, dim=0)
                    ci = ci + (k0 - k_lo)
                    if top2:
                        t = torch.topk(val, 2, dim=0)[0] if val.shape[0] > 1 else torch.cat([val, torch.zeros_like(val)])
                        # the second largest of both chunks: the smaller of the two maxima, or either chunk's own second
                        second = t[1] if mv is None else torch.maximum(torch.minimum(mv, cv), torch.maximum(second, t[1]))
                    if mv is None:
                        mv, mi = cv, ci
                    else:
                        mi = torch.where(cv > mv, ci, mi)
                        mv = torch.maximum(mv, cv)
                out[side].append(mv)
                idx[side].append(mi)
                if top2:
                    gap[side].append(mv - second)
        img = torch.stack([torch.cat(out[0]).view(w, w), torch.cat(out[1]).view(w, w)])
        imgs.append((img - 0.5) / 0.5)
        amax.append(torch.stack([torch.cat(idx[0]).view(w, w), torch.cat(idx[1]).view(w, w)]))
        if top2:
            gaps.append(torch.stack([torch.cat(gap[0]).view(w, w), torch.cat(gap[1]).view(w, w)]))
    res = (torch.stack(imgs), torch.stack(amax), ranges)
    return res + (torch.stack(gaps),) if top2 else res


def backward(src_pred, tgt, dimgs, argmax, rho=24, w=64, eulers=None, dtype=torch.float64):
    """d(sum dimgs * imgs)/d src_pred with each source pixel's gradient routed to argmax[v, 0, pixel] (-1: none); dmin / dmax are
    constants, as the reference's .item() makes them."""
    eulers = view_eulers("muti") if eulers is None else eulers
    n = src_pred.shape[0]
    x = torch.cat([src_pred, tgt], dim=0).to(dtype)
    pix_xy = pixel_centres(w, dtype, x.device)
    grad = torch.zeros(n, 3, dtype=dtype, device=x.device)
    for v, e in enumerate(eulers):
        R = rotation_matrix(e).to(device=x.device, dtype=dtype)
        X = _rotate(R, x, dtype)
        dmin, dmax = X[:, 2].min().item(), X[:, 2].max().item()
        a = argmax[v, 0].reshape(-1).to(x.device).long()
        sel = a >= 0
        k, c = a[sel], pix_xy[sel]
        up = dimgs[v, 0].reshape(-1).to(device=x.device, dtype=dtype)[sel]
        Xk = X[k]
        pv = 1 - (Xk[:, 2] - dmin) / (dmax - dmin)
        d = Xk[:, :2] - c
        g = torch.exp(-(d ** 2).sum(dim=1) / 2 * rho ** 2)
        dX = torch.zeros(k.shape[0], 3, dtype=dtype, device=x.device)
        dX[:, :2] = (-2 * rho ** 2 * up * pv * g)[:, None] * d
        dX[:, 2] = -2 * up * g / (dmax - dmin)
        gv = torch.zeros(n, 3, dtype=dtype, device=x.device).index_add_(0, k, dX)
        grad += gv @ R
    return grad
