"""Host side of the class-location feature without a device: the library's argument checks and size query
(csrc/class_locations.hip), the numpy emulation of hip_backend.class_locations against the one-line oracle, and
seg_utils.sample_class_locations on that emulation."""
import ctypes as C

import numpy as np
import pytest
import torch

import class_locations_emu as emu
import class_locations_oracle as co
from rehrseg_amd import lib as L

OK_EHIP, EINVAL, ENOSUP = -3, -1, -2      # an accepted call meets "no device" (REHR_EHIP)
N0, R0 = 5000, 7
WS0 = 16                                   # two chunks of 4096: 8 bytes, rounded up to 16

# (row, arguments replaced on the well-formed call, code).  Pointers are dummies that nothing on the host dereferences.
_BASE = dict(label=0x10000, N=N0, value=1, u=0x20000, R=R0, count=0x30000, index=0x40000, ws=0x50000, ws_bytes=WS0)
_ROWS = [
    ("well formed", {}, OK_EHIP),
    ("value -1", dict(value=-1), OK_EHIP),
    ("value 0", dict(value=0), OK_EHIP),
    ("value 255", dict(value=255), OK_EHIP),
    ("a roomier workspace", dict(ws_bytes=4096), OK_EHIP),
    ("N = 2^31 - 1", dict(N=2**31 - 1, ws_bytes=4 * 2**19), OK_EHIP),
    ("R = 2^20", dict(R=2**20), OK_EHIP),
    ("null label", dict(label=None), EINVAL),
    ("null u", dict(u=None), EINVAL),
    ("null count", dict(count=None), EINVAL),
    ("null index", dict(index=None), EINVAL),
    ("null workspace", dict(ws=None), EINVAL),
    ("N = 0", dict(N=0), EINVAL),
    ("N = -1", dict(N=-1), EINVAL),
    ("R = 0", dict(R=0), EINVAL),
    ("R = -1", dict(R=-1), EINVAL),
    ("value -2", dict(value=-2), EINVAL),
    ("value 256", dict(value=256), EINVAL),
    ("label off 16 bytes", dict(label=0x10008), EINVAL),
    ("u off 4 bytes", dict(u=0x20002), EINVAL),
    ("index off 4 bytes", dict(index=0x40002), EINVAL),
    ("count off 8 bytes", dict(count=0x30004), EINVAL),
    ("workspace off 16 bytes", dict(ws=0x50008), EINVAL),
    ("workspace one byte short", dict(ws_bytes=WS0 - 1), EINVAL),
    ("five chunks need 32 bytes", dict(N=4 * 4096 + 1, ws_bytes=16), EINVAL),
    ("five chunks in 32 bytes", dict(N=4 * 4096 + 1, ws_bytes=32), OK_EHIP),
    ("N = 2^31", dict(N=2**31, ws_bytes=4 * 2**19 + 16), ENOSUP),
    ("R = 2^20 + 1", dict(R=2**20 + 1), ENOSUP),
]


def _call(lib, a):
    return lib.rehr_class_locations_u8(a["label"], a["N"], a["value"], a["u"], a["R"], a["count"], a["index"], a["ws"],
                                       a["ws_bytes"], None)


def test_validation_codes_without_a_device():
    """Runs only where there is no device: an accepted call then meets "no device", not a launch on dummy pointers."""
    if torch.cuda.is_available():
        pytest.skip("dummy pointers: only where an accepted call cannot be launched")
    lib = L.load()
    assert lib.rehr_class_locations_workspace_bytes(N0) == WS0
    for name, over, want in _ROWS:
        assert _call(lib, dict(_BASE, **over)) == want, name


def test_size_query():
    q = L.load().rehr_class_locations_workspace_bytes
    assert q.restype is C.c_int64
    sizes = [1, 15, 16, 17, co.W, co.C - 1, co.C, co.C + 1, 4 * co.C, 4 * co.C + 1, 20 * 455 * 633, 2**31 - 1]
    got = [q(n) for n in sizes]
    for n, b in zip(sizes, got):
        chunks = (n + co.C - 1) // co.C
        assert b == (4 * chunks + 15) // 16 * 16 and b % 16 == 0 and b >= 16, (n, b)
    assert got == sorted(got)                                   # monotone in N
    assert q(0) == EINVAL and q(-5) == EINVAL and q(2**31) == ENOSUP


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("N", co.SIZES)
def test_emulation_equals_the_oracle(N):
    label = co.mixed_run(N, N)
    u = co.fractions(65, N + 1)
    for value in co.VALUES + (0,):
        want_count, want = co.oracle(label, value, u)
        count, index = emu.class_locations(_t(label), value, _t(u.view(np.int32)))
        assert int(count[0]) == want_count and np.array_equal(index.numpy(), want), (N, value)


def test_emulation_skips_empty_chunks_and_reports_no_match():
    label = np.zeros(6 * co.C + 3, np.uint8)
    label[5], label[5 * co.C + 7], label[-1] = 1, 1, 1          # chunks 1..4 are empty
    u = co.fractions(64, 3)
    count, index = emu.class_locations(_t(label), 1, _t(u.view(np.int32)))
    assert int(count[0]) == 3 and np.array_equal(index.numpy(), co.oracle(label, 1, u)[1])
    assert set(index.numpy().tolist()) == {5, 5 * co.C + 7, label.size - 1}
    count, index = emu.class_locations(_t(label), 2, _t(u.view(np.int32)))
    assert int(count[0]) == 0 and (index.numpy() == -1).all()


@pytest.fixture
def on_emulation():
    from rehrseg_amd import ops
    old = ops.set_backend(emu)
    yield
    ops.set_backend(old)


def _volume(seed=0, shape=(9, 14, 11)):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 1, 2, 255], np.uint8), size=shape, p=[0.9, 0.05, 0.03, 0.02])


def test_sample_class_locations(on_emulation):
    from rehrseg_amd.utils.seg_utils import sample_class_locations
    lab = _volume()
    t = sample_class_locations(lab, classes=(1, 2, 7, -1), n=300, seed=5, device="cpu")
    assert list(t) == [1, 2, 7, -1]
    for c in (1, 2, -1):
        a = t[c]
        assert a.dtype == np.int64 and a.shape == (300, 3)
        assert (a >= 0).all() and (a < np.array(lab.shape)).all()
        at = lab[a[:, 0], a[:, 1], a[:, 2]]
        assert (at != 0).all() if c == -1 else (at == c).all()
        u = np.random.default_rng(5).integers(0, 2**32, 300, dtype=np.uint32)
        assert np.array_equal(np.ravel_multi_index(tuple(a.T), lab.shape), co.oracle(lab, c, u)[1])
    assert t[7].shape == (0, 3) and t[7].dtype == np.int64
    again = sample_class_locations(torch.from_numpy(lab), classes=(1, 2, 7, -1), n=300, seed=5, device="cpu")
    assert all(np.array_equal(again[c], t[c]) for c in t)
    other = sample_class_locations(lab, classes=(1,), n=300, seed=6, device="cpu")
    assert not np.array_equal(other[1], t[1])


def test_sample_class_locations_of_a_list(on_emulation):
    from rehrseg_amd.utils.seg_utils import sample_class_locations
    vols = [_volume(1), np.zeros((4, 5, 6), np.uint8), _volume(2, (5, 6, 7))]
    got = sample_class_locations(vols, classes=(1, 255), n=50, seed=3, device="cpu")
    assert isinstance(got, list) and len(got) == 3
    assert got[1][1].shape == (0, 3) and got[1][255].shape == (0, 3)
    for i in (0, 2):                                             # volume i is drawn with seed + i
        single = sample_class_locations(vols[i], classes=(1, 255), n=50, seed=3 + i, device="cpu")
        assert all(np.array_equal(got[i][c], single[c]) for c in (1, 255))
    with pytest.raises(ValueError):
        sample_class_locations(vols[0], classes=(300,), device="cpu")
    with pytest.raises(ValueError):
        sample_class_locations(vols[0], n=0, device="cpu")
