"""Volumes and readers shared by the foreground-oversampling tests of TrainSetMultipleSegSREfficient (test only).
The image of a subject holds 1 + its own linear voxel index (exact in fp32 below 2**24; 0 is the constant pad), so
the smallest positive value of a gathered patch names the crop's origin corner, with or without flips."""
import numpy as np
import torch

from feed_cases import emu_axis_resample, emu_patch_gather

SHAPE, PATCH, SEP = (40, 36, 24), (16, 16, 4), 2
EXT = (PATCH[0], PATCH[1], PATCH[2] * SEP)
LESION = ((39, 35, 23), (38, 35, 23), (39, 34, 23))     # 3 voxels in the far corner


def subject(shape=SHAPE, lesion=(), value=1):
    n = int(np.prod(shape))
    assert n < 2**24
    seg = np.zeros(shape, np.uint8)
    for v in lesion:
        seg[v] = value
    return {"img": (np.arange(n, dtype=np.float32) + 1).reshape(shape), "seg": seg}


def two_subjects():
    """One subject with the 3-voxel lesion in a corner, one without foreground."""
    return [subject(lesion=LESION), subject()]


def make(volumes, device, patch=PATCH, **kw):
    from rehrseg_amd.utils.train_set import TrainSetMultipleSegSREfficient
    return TrainSetMultipleSegSREfficient(None, list(range(len(volumes))), float(SEP), 1.0, patch, None, norm=False,
                                          device=device, volumes=volumes, **kw)


def emulate(monkeypatch):
    """The feed's two launches and the class-location launch on their numpy emulations, volumes on the CPU."""
    import class_locations_emu
    from rehrseg_amd import hip_backend as hb
    from rehrseg_amd import ops
    from rehrseg_amd.utils import train_set as ts
    monkeypatch.setattr(hb, "patch_gather", emu_patch_gather)
    monkeypatch.setattr(hb, "axis_resample", emu_axis_resample)
    monkeypatch.setattr(ts._DeviceSet, "_check_device", lambda self, device: torch.device("cpu"))
    monkeypatch.setattr(ops, "_backend", class_locations_emu)


def origin_of(data, shape=SHAPE):
    """The crop origin (x0, y0, z0) from an item's image patch (1, z, y, x).  The patch holds every SEP-th slice of the
    crop, counted from the crop's first slice, or from its last one when the z axis is flipped: then the lowest slice
    it holds is z0 + SEP - 1 (the crop's z extent is a multiple of SEP)."""
    a = data.detach().cpu().numpy()
    low = np.where(a > 0, a, np.inf)
    _, _, yi, xi = np.unravel_index(int(np.argmin(low)), a.shape)
    x0, y0, z_low = (int(c) for c in np.unravel_index(int(low.min()) - 1, shape))
    column = a[0, :, yi, xi]
    column = column[column > 0]
    flipped = column.size > 1 and column[0] > column[-1]
    return x0, y0, z_low - (SEP - 1 if flipped else 0)


def clamp_origin(voxel, shape=SHAPE, ext=EXT):
    return tuple(min(max(int(c) - e // 2, 0), max(s - e, 0)) for c, s, e in zip(voxel, shape, ext))


def inside(voxel, origin, ext=EXT):
    return all(o <= int(c) < o + e for c, o, e in zip(voxel, origin, ext))
