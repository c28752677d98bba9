"""The oracle of rehr_class_locations_u8 (test only): one numpy line over the whole label run, and the label runs and
fraction sets the tests share.  C and W are the chunk and the wave step of csrc/class_locations.hip as built."""
import numpy as np

C, W = 4096, 1024          # voxels per block step of the count pass / per wave step of the select pass
VALUES = (1, 2, 255, -1)


def match_of(label, value):
    flat = np.asarray(label, dtype=np.uint8).reshape(-1)
    return flat != 0 if value == -1 else flat == np.uint8(value)


def oracle(label, value, u):
    """(count, index int32 [R]): index[j] = the ((u[j] * count) >> 32)-th matching voxel, all -1 without a match."""
    match = match_of(label, value)
    u = np.asarray(u, dtype=np.uint32)
    count = int(match.sum())
    if count == 0:
        return 0, np.full(u.shape, -1, np.int32)
    return count, np.flatnonzero(match)[(u.astype(np.uint64) * np.uint64(count)) >> np.uint64(32)].astype(np.int32)


def fractions(R, seed):
    """R fractions that hold 0 and 2**32 - 1 (rank 0 and rank count - 1) when there is room for them."""
    u = np.random.default_rng(seed).integers(0, 2**32, R, dtype=np.uint32)
    u[0] = 0
    if R > 1:
        u[-1] = 2**32 - 1
    return u


def mixed_run(N, seed):
    """Labels 0, 1, 2 and 255 mixed: about 70 % background (a signed-byte compare would miss 255)."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 1, 2, 255], np.uint8), size=N, p=[0.7, 0.1, 0.1, 0.1])


SIZES = (1, 15, 16, 17, W - 1, W, W + 1, C - 1, C, C + 1, 3 * C + 5)
