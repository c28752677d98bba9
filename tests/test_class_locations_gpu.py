"""rehr_class_locations_u8 on the device against the one-line numpy oracle (tests/class_locations_oracle.py): exact
integers everywhere.  The shapes are the smallest at which the kernel takes another path: around one 16-byte vector,
one wave step W, one chunk C, several chunks with a tail, and one small volume."""
import numpy as np
import pytest
import torch

import class_locations_oracle as co
from rehrseg_amd import hip_backend as hb
from rehrseg_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, PATTERN = 4096, 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u(u):
    return _dev(np.asarray(u, np.uint32).view(np.int32))


def _check(label, value, u, what=""):
    """One call against the oracle; returns the oracle's count."""
    lab = _dev(label)
    before = lab.clone()
    count, index = hb.class_locations(lab, value, _u(u))
    want_count, want = co.oracle(label, value, u)
    assert count.dtype == torch.int64 and count.shape == (1,) and index.dtype == torch.int32
    assert int(count.cpu()[0]) == want_count, (what, value)
    got = index.cpu().numpy()
    assert np.array_equal(got, want), (what, value, np.flatnonzero(got != want)[:8])
    assert torch.equal(lab, before), "the label run was written"
    return want_count


@pytest.mark.parametrize("N", co.SIZES)
def test_mixed_labels_every_value(N):
    label = co.mixed_run(N, 100 + N)
    u = co.fractions(65, N)
    for value in co.VALUES + (0,):
        _check(label, value, u, f"N={N}")


def test_small_volume():
    label = co.mixed_run(20 * 61 * 67, 7).reshape(20, 61, 67)
    u = co.fractions(4097, 8)
    for value in co.VALUES:
        assert _check(label, value, u, "volume") > 0


@pytest.mark.parametrize("N", [1, 17, co.W + 1, co.C, 3 * co.C + 5])
def test_where_the_matches_lie(N):
    u = co.fractions(64, N)
    first, last, every = np.zeros(N, np.uint8), np.zeros(N, np.uint8), np.full(N, 255, np.uint8)
    first[0], last[-1] = 255, 255
    assert _check(first, 255, u, "first voxel") == 1
    assert _check(last, 255, u, "last voxel") == 1
    assert _check(every, 255, u, "every voxel") == N
    assert _check(every, -1, u, "every voxel, any") == N
    assert _check(every, 1, u, "no match") == 0
    assert _check(np.zeros(N, np.uint8), -1, u, "all background") == 0
    if N % 16:
        tail = np.zeros(N, np.uint8)
        tail[N - N % 16:] = 2
        assert _check(tail, 2, u, "tail bytes only") == N % 16
        assert _check(tail, -1, u, "tail bytes only, any") == N % 16


def test_rank_zero_and_rank_count_minus_one():
    label = co.mixed_run(3 * co.C + 5, 11)
    u = np.array([0, 2**32 - 1, 0, 2**32 - 1], np.uint32)
    for value in co.VALUES:
        lab = _dev(label)
        count, index = hb.class_locations(lab, value, _u(u))
        at = np.flatnonzero(co.match_of(label, value))
        assert int(count.cpu()[0]) == at.size
        assert index.cpu().numpy().tolist() == [at[0], at[-1], at[0], at[-1]]


def test_runs_of_empty_chunks():
    """Equal prefixes: the chunks between the populated ones hold nothing and must never be chosen."""
    label = np.zeros(9 * co.C + 3, np.uint8)
    where = [5, co.C - 1, 4 * co.C, 4 * co.C + co.W + 1, 9 * co.C + 2]      # chunks 0, 4 and 9 (the tail)
    label[where] = 1
    u = np.concatenate([co.fractions(60, 13), (np.arange(5, dtype=np.uint64) * 2**32 // 5 + 1).astype(np.uint32)])
    assert _check(label, 1, u, "empty chunks") == 5
    got = hb.class_locations(_dev(label), 1, _u(u))[1].cpu().numpy()
    assert set(got.tolist()) == set(where)
    lead = np.zeros(5 * co.C, np.uint8)                                     # empty chunks in front and behind
    lead[2 * co.C + 100] = 7
    assert _check(lead, 7, u, "empty chunks in front") == 1


@pytest.mark.parametrize("R", [1, 64, 65, 4097])
def test_number_of_fractions(R):
    label = co.mixed_run(2 * co.C + 9, 17)
    u = co.fractions(R, R)
    _check(label, 1, u, f"R={R}")
    _check(label, -1, u, f"R={R}")


def test_two_runs_give_identical_bits():
    label = _dev(co.mixed_run(20 * 61 * 67, 19))
    u = _u(co.fractions(4097, 20))
    a = hb.class_locations(label, -1, u)
    b = hb.class_locations(label, -1, u)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("N", [17, co.C, 4 * co.C + 1, 20 * 61 * 67])
def test_exact_size_workspace_and_guarded_outputs(N):
    """An exact-size workspace with guard bytes behind it, and guard words around count and index, stay intact."""
    label = co.mixed_run(N, 23)
    lab, u_np = _dev(label), co.fractions(65, 24)
    u = _u(u_np)
    n = int(L.load().rehr_class_locations_workspace_bytes(N))
    assert n > 0 and n % 16 == 0
    buf = torch.full((n + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    ws = buf[:n]
    assert ws.data_ptr() % 16 == 0
    out = torch.full((4 + 65 + 4,), -7, dtype=torch.int32, device=DEV)
    cnt = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    count, index = hb.class_locations(lab, 1, u, count=cnt[1:2], index=out[4:69], workspace=ws)
    torch.cuda.synchronize()
    assert bool((buf[n:] == PATTERN).all()), "the kernels wrote past the queried size"
    assert cnt[0] == -7 and cnt[2] == -7 and bool((out[:4] == -7).all()) and bool((out[69:] == -7).all())
    want_count, want = co.oracle(label, 1, u_np)
    assert int(cnt[1]) == want_count and np.array_equal(out[4:69].cpu().numpy(), want)
    roomy = hb.class_locations(lab, 1, u)
    assert torch.equal(roomy[0], count) and torch.equal(roomy[1], index)


def test_wrapper_refuses_what_the_library_would():
    lab = _dev(co.mixed_run(64, 1))
    u = _u(co.fractions(4, 1))
    with pytest.raises(L.RehrsegHipError):
        hb.class_locations(lab, 256, u)
    with pytest.raises(L.RehrsegHipError):
        hb.class_locations(lab.cpu(), 1, u)
    with pytest.raises(L.RehrsegHipError):
        hb.class_locations(lab[1:], 1, u)               # not 16-byte aligned: REHR_EINVAL from the library
    with pytest.raises(L.RehrsegHipError):
        hb.class_locations(lab, 1, u.to(torch.int64))
