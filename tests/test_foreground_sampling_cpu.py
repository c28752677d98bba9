"""Foreground oversampling of TrainSetMultipleSegSREfficient on the emulated feed: the default keeps today's draw
protocol bit for bit, a forced item centres its crop on a voxel of the class-location table, `batch` forces by
position and `__getitem__` by one extra draw."""
import random

import numpy as np
import pytest
import torch

import foreground_cases as fc


@pytest.fixture
def emulated(monkeypatch):
    fc.emulate(monkeypatch)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert x.dtype == y.dtype and torch.equal(x, y)
        else:
            assert x == y


@pytest.mark.parametrize("flip", [False, True])
def test_default_and_zero_keep_the_draw_protocol(emulated, flip):
    vols = fc.two_subjects()
    plain = fc.make(vols, "cpu", random_flip=flip)
    zero = fc.make(vols, "cpu", random_flip=flip, oversample_foreground=0.0, foreground_classes=(1, 2),
                   foreground_samples=50, foreground_seed=9)
    assert zero._locations is None                                   # no table is built
    random.seed(4)
    a = [plain[k % 2] for k in range(6)] + [plain.batch([0, 1, 1, 0])]
    state_a = random.getstate()
    random.seed(4)
    b = [zero[k % 2] for k in range(6)] + [zero.batch([0, 1, 1, 0])]
    assert random.getstate() == state_a                              # the same number of draws
    for x, y in zip(a, b):
        _same(x, y)
    # today's protocol itself: three randint draws, then one random() per axis when flipping
    random.seed(4)
    item = plain[0]
    after = random.getstate()
    random.seed(4)
    want = tuple(random.randint(0, s - e) for s, e in zip(fc.SHAPE, fc.EXT))
    if flip:
        [random.random() for _ in range(3)]
    assert random.getstate() == after and fc.origin_of(item[0]) == want


def _tables(vols, classes, n, seed):
    from rehrseg_amd.utils.seg_utils import sample_class_locations
    return sample_class_locations([v["seg"] for v in vols], classes, n, seed, device="cpu")


@pytest.mark.parametrize("flip", [False, True])
def test_forced_items_obey_the_clamp_formula(emulated, flip):
    rng = np.random.default_rng(1)
    seg_voxels = [tuple(int(c) for c in v) for v in rng.integers(0, fc.SHAPE, size=(12, 3))] + [(0, 0, 0), fc.LESION[0]]
    vols = [fc.subject(lesion=seg_voxels)]
    ds = fc.make(vols, "cpu", random_flip=flip, oversample_foreground=1.0, foreground_samples=64, foreground_seed=2)
    table = _tables(vols, (1,), 64, 2)[0][1]
    assert table.shape == (64, 3) and {tuple(v) for v in table.tolist()} <= set(seg_voxels)
    random.seed(0)
    seen = set()
    for k in range(24):
        item = ds[0] if k % 2 else tuple(o[0] if torch.is_tensor(o) else o for o in ds.batch([0]))
        origin = fc.origin_of(item[0])
        hits = [v for v in table.tolist() if fc.clamp_origin(v) == origin]
        assert hits and all(fc.inside(v, origin) for v in hits), (k, origin)
        assert float(item[2].sum()) > 0
        seen.add(origin)
    assert len(seen) > 3                                              # the table is drawn from, not one voxel


def test_forced_item_of_a_volume_thinner_than_the_patch(emulated):
    shape = (40, 10, 24)                                              # 10 < 16 on the second axis
    vols = [fc.subject(shape, lesion=[(3, 9, 20), (30, 0, 2)])]
    ds = fc.make(vols, "cpu", oversample_foreground=1.0, foreground_samples=16)
    table = _tables(vols, (1,), 16, 0)[0][1]
    random.seed(3)
    for _ in range(8):
        item = ds[0]
        assert tuple(item[0].shape) == (1, fc.PATCH[2], fc.PATCH[1], fc.PATCH[0])
        origin = fc.origin_of(item[0], shape)
        assert origin[1] == 0
        hits = [v for v in table.tolist() if fc.clamp_origin(v, shape) == origin]
        assert hits and all(fc.inside(v, origin) for v in hits)
        assert float(item[2].sum()) > 0


FIRST_FORCED = {(2, 0.33): 1, (3, 0.33): 2, (4, 0.33): 3, (8, 0.33): 5, (2, 0.5): 1, (3, 0.5): 2, (4, 0.5): 2, (8, 0.5): 4}


@pytest.mark.parametrize("B,p", sorted(FIRST_FORCED))
def test_batch_forces_by_position(emulated, B, p):
    """The lesion sits in the far corner: only the crop with the largest origin holds it, which a uniform draw at this
    seed does not produce (checked first), so an item holds foreground iff it was forced."""
    assert FIRST_FORCED[(B, p)] == round(B * (1 - p))
    vols = fc.two_subjects()[:1]
    seed = 12
    uniform = fc.make(vols, "cpu")
    random.seed(seed)
    assert float(uniform.batch([0] * B)[2].sum()) == 0                # the seed's uniform draws all miss the lesion
    state_uniform = random.getstate()
    ds = fc.make(vols, "cpu", oversample_foreground=p, foreground_samples=32)
    random.seed(seed)
    out = ds.batch([0] * B)
    has = [float(out[2][j].sum()) > 0 for j in range(B)]
    assert has == [j >= FIRST_FORCED[(B, p)] for j in range(B)]
    for j in range(B):
        if has[j]:
            assert fc.origin_of(out[0][j]) == fc.clamp_origin(fc.LESION[0])
    assert random.getstate() != state_uniform                         # the forced items drew something else


def test_getitem_draws_once_before_the_origin(emulated):
    vols = fc.two_subjects()[:1]
    p = 0.5
    ds = fc.make(vols, "cpu", oversample_foreground=p, foreground_samples=32)
    table = _tables(vols, (1,), 32, 0)[0][1]
    random.seed(21)
    items = [ds[0] for _ in range(12)]
    end = random.getstate()
    random.seed(21)
    forced = []
    for item in items:
        f = random.random() < p
        forced.append(f)
        if f:
            want = fc.clamp_origin(table[random.randrange(len(table))])
        else:
            want = tuple(random.randint(0, s - e) for s, e in zip(fc.SHAPE, fc.EXT))
        assert fc.origin_of(item[0]) == want
    assert random.getstate() == end and True in forced and False in forced


def test_subject_without_foreground_falls_back_to_uniform(emulated):
    vols = fc.two_subjects()
    plain = fc.make(vols, "cpu", random_flip=True)
    ds = fc.make(vols, "cpu", random_flip=True, oversample_foreground=1.0, foreground_samples=8)
    assert ds._locations[1] == []
    random.seed(5)
    want = plain.batch([1, 1, 1])
    random.seed(5)
    _same(ds.batch([1, 1, 1]), want)                                  # batch makes no extra draw
    random.seed(5)
    random.random()                                                   # __getitem__'s one extra draw
    want = plain[1]
    random.seed(5)
    _same(ds[1], want)


def test_several_classes_choose_among_those_present(emulated):
    a = fc.subject(lesion=[(2, 3, 4)], value=2)                       # class 2 only
    b = fc.subject(lesion=[(2, 3, 4)], value=1)
    b["seg"][30, 30, 20] = 2                                          # both classes
    ds = fc.make([a, b], "cpu", oversample_foreground=1.0, foreground_classes=(1, 2), foreground_samples=8)
    assert [c for c, _ in ds._locations[0]] == [2] and [c for c, _ in ds._locations[1]] == [1, 2]
    random.seed(8)
    for _ in range(4):
        assert fc.origin_of(ds[0][0]) == fc.clamp_origin((2, 3, 4))
    got = {fc.origin_of(ds[1][0]) for _ in range(16)}
    assert got == {fc.clamp_origin((2, 3, 4)), fc.clamp_origin((30, 30, 20))}


@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan")])
def test_probability_outside_the_unit_interval(emulated, p):
    with pytest.raises(ValueError):
        fc.make(fc.two_subjects(), "cpu", oversample_foreground=p)
