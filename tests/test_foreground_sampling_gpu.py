"""Foreground oversampling of TrainSetMultipleSegSREfficient on the device: two subjects of 40x36x24, patches of
(16, 16, 4) at separation 2, one subject with a 3-voxel lesion in a corner and one without foreground."""
import random
import warnings

import numpy as np
import pytest
import torch

import foreground_cases as fc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _count_syncs(fn):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return out, [w for w in rec if "called a synchronizing" in str(w.message)]


def _resident(volumes):
    """The volumes as a stage2_volumes-style list of dicts of device tensors."""
    return [{"img": torch.from_numpy(v["img"]).to(DEV), "seg": torch.from_numpy(v["seg"]).to(DEV)} for v in volumes]


def test_every_forced_item_holds_the_lesion():
    ds = fc.make(fc.two_subjects(), DEV, random_flip=True, oversample_foreground=1.0, foreground_samples=64)
    random.seed(1)
    for _ in range(32):
        data, seg, seg_sr, _ = ds[0]
        assert float(seg_sr.sum()) > 0
        assert fc.origin_of(data) == fc.clamp_origin(fc.LESION[0])       # the three voxels clamp to one origin
    batch = ds.batch([0] * 8)
    assert bool((batch[2].sum(dim=(1, 2, 3, 4)) > 0).all())
    for _ in range(4):                                                   # no foreground: the uniform draws, no error
        data, seg, seg_sr, _ = ds[1]
        assert float(seg_sr.sum()) == 0 and tuple(data.shape) == (1, fc.PATCH[2], fc.PATCH[1], fc.PATCH[0])
    assert float(ds.batch([1, 0, 1])[2][1].sum()) > 0


def test_table_on_the_device_equals_the_emulation(monkeypatch):
    from rehrseg_amd.utils.seg_utils import sample_class_locations
    rng = np.random.default_rng(3)
    labels = [rng.choice(np.array([0, 1, 2], np.uint8), size=fc.SHAPE, p=[0.98, 0.01, 0.01]), np.zeros(fc.SHAPE, np.uint8)]
    got = sample_class_locations([torch.from_numpy(a).to(DEV) for a in labels], (1, 2, -1), 500, 4)
    host = sample_class_locations(labels, (1, 2, -1), 500, 4, device=DEV)   # uploaded: the same table
    with monkeypatch.context() as m:
        fc.emulate(m)
        want = sample_class_locations(labels, (1, 2, -1), 500, 4, device="cpu")
    for g, h, w in zip(got, host, want):
        for c in (1, 2, -1):
            assert g[c].dtype == np.int64 and np.array_equal(g[c], w[c]) and np.array_equal(h[c], w[c])
    assert got[0][1].shape == (500, 3) and got[1][1].shape == (0, 3)


@pytest.mark.parametrize("flip", [False, True])
def test_default_equals_the_emulated_cpu_run(monkeypatch, flip):
    vols = fc.two_subjects()
    with monkeypatch.context() as m:
        fc.emulate(m)
        cpu = fc.make(vols, "cpu", random_flip=flip)
        random.seed(6)
        want = [cpu[k % 2] for k in range(6)] + [cpu.batch([0, 1, 1])]
    ds = fc.make(vols, DEV, random_flip=flip)
    random.seed(6)
    got = [ds[k % 2] for k in range(6)] + [ds.batch([0, 1, 1])]
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            if torch.is_tensor(a):
                assert a.is_cuda and a.dtype == b.dtype and torch.equal(a.cpu(), b)
            else:
                assert a == b


def test_construction_makes_one_host_sync_and_batch_none():
    vols = _resident(fc.two_subjects())
    fc.make(vols, DEV, oversample_foreground=0.33, foreground_samples=64)    # warm-up: library, allocator
    torch.cuda.synchronize()
    ds, syncs = _count_syncs(lambda: fc.make(vols, DEV, oversample_foreground=0.33, foreground_samples=64))
    assert len(syncs) == 1, [str(w.message) for w in syncs]                  # the one download of all tables
    # the resident labels are used where they lie: no copy, and no download (it would be a second sync)
    assert all(lab.data_ptr() == v["seg"].data_ptr() for lab, v in zip(ds.labels, vols))
    assert len(ds._locations[0]) == 1 and ds._locations[0][0][1].shape == (64, 3) and ds._locations[1] == []
    random.seed(2)
    ds.batch([0, 1, 0])                                                      # warm-up
    torch.cuda.synchronize()
    out, syncs = _count_syncs(lambda: ds.batch([0, 1, 0]))
    assert len(syncs) == 0, [str(w.message) for w in syncs]
    assert float(out[2][2].sum()) > 0                                        # item 2 of 3 is the forced one
    _, syncs = _count_syncs(lambda: fc.make(vols, DEV))
    assert len(syncs) == 0, [str(w.message) for w in syncs]                  # without the option: no table, no sync
