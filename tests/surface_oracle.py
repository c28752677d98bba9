"""Brute-force fp64 yardstick of the boundary metrics (test only; independent of the kernels and of their emulation).

Surfaces by shifted ANDs, the distance of every surface voxel of one map to the surface of the other as the minimum
over ALL surface pairs in fp64 (numpy on the host, or chunked torch fp64 on a device for a large case), then hd, hd95
(numpy.percentile) and assd as DESIGN section 3.15 defines them.  The spacing is the fp32-rounded value widened to
fp64: the value the kernels use."""
import numpy as np

TOL = 6.0 * 2.0 ** -24    # relative, per distance and per metric: the derivation is in tests/test_surface_gpu.py


def surface(mask):
    """Foreground voxels with a background face neighbour; outside the volume is background."""
    m = np.asarray(mask) != 0
    p = np.pad(m, 1)
    covered = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] &
               p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return m & ~covered


def _spacing(spacing):
    return np.asarray(spacing, dtype=np.float32).astype(np.float64)


def _pair_minima_numpy(a, b, sp, chunk=512):
    """a (na, 3), b (nb, 3) voxel indices as fp64, sp (3,) -> (min over b for every a, min over a for every b)."""
    to_b = np.empty(len(a))
    to_a = np.full(len(b), np.inf)
    for lo in range(0, len(a), chunk):
        d = (a[lo:lo + chunk, None, :] - b[None, :, :]) * sp
        d2 = d[..., 0] ** 2 + d[..., 1] ** 2 + d[..., 2] ** 2
        to_b[lo:lo + chunk] = d2.min(1)
        to_a = np.minimum(to_a, d2.min(0))
    return np.sqrt(to_b), np.sqrt(to_a)


def _pair_minima_torch(a, b, sp, device, chunk=1024):
    import torch
    s0, s1, s2 = (float(v) for v in sp)
    a = torch.from_numpy(a).to(device)
    b = torch.from_numpy(b).to(device)
    to_b = torch.empty(len(a), dtype=torch.float64, device=device)
    to_a = torch.full((len(b),), float("inf"), dtype=torch.float64, device=device)
    for lo in range(0, len(a), chunk):
        c = a[lo:lo + chunk]
        d2 = (((c[:, None, 0] - b[None, :, 0]) * s0) ** 2 + ((c[:, None, 1] - b[None, :, 1]) * s1) ** 2 +
              ((c[:, None, 2] - b[None, :, 2]) * s2) ** 2)
        to_b[lo:lo + chunk] = d2.min(1).values
        to_a = torch.minimum(to_a, d2.min(0).values)
    return to_b.sqrt().cpu().numpy(), to_a.sqrt().cpu().numpy()


def metrics(pred, gt, spacing=(1., 1., 1.), device=None):
    """{'n_pred', 'n_gt', 's_pg', 's_gp' (ascending fp64 distances), 'hd', 'hd95', 'assd'} of two (D, H, W) maps.
    `device`: run the pair minima as chunked torch fp64 there (the large case) instead of numpy on the host."""
    sp = _spacing(spacing)
    a = np.argwhere(surface(pred)).astype(np.float64)
    b = np.argwhere(surface(gt)).astype(np.float64)
    out = {"n_pred": len(a), "n_gt": len(b)}
    if len(a) == 0 or len(b) == 0:
        out.update(s_pg=np.empty(0), s_gp=np.empty(0), hd=float("nan"), hd95=float("nan"), assd=float("nan"))
        return out
    s_pg, s_gp = _pair_minima_numpy(a, b, sp) if device is None else _pair_minima_torch(a, b, sp, device)
    out.update(s_pg=np.sort(s_pg), s_gp=np.sort(s_gp), hd=float(max(s_pg.max(), s_gp.max())),
               hd95=float(np.percentile(np.concatenate([s_pg, s_gp]), 95)),
               assd=float((s_pg.mean() + s_gp.mean()) / 2))
    return out


def ellipsoid(shape, centre, radii):
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    return (((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 +
            ((x - centre[2]) / radii[2]) ** 2) <= 1


def pinned_case():
    """The pinned pair of the design section: (P, G, spacing, expected)."""
    shape = (6, 20, 24)
    P = ellipsoid(shape, (2.5, 9, 11), (2.2, 6, 7))
    G = ellipsoid(shape, (3, 11, 9), (2.6, 5, 8))
    want = {"n_pred": 238, "n_gt": 250, "hd": 5.315072906367325, "hd95": 5.0, "assd": 1.1624448587540757}
    return P, G, (5.0, 0.5, 0.75), want
