"""CPU statement of hip_backend.class_locations (test only): the passes of csrc/class_locations.hip in numpy over CPU
tensors -- one count per chunk of 4096 voxels, their exclusive prefix, the last chunk whose prefix is <= the rank
(searchsorted side='right'), the k-th match inside that chunk.  Everything else is tests/intensity_emu.py's; install it
with ops.set_backend()."""
import numpy as np
import torch

import intensity_emu

name = "class_locations_emu"
CHUNK = 4096


def __getattr__(attr):
    return getattr(intensity_emu, attr)


def class_locations_workspace(N, device):
    return torch.empty((((N + CHUNK - 1) // CHUNK) * 4 + 15) // 16 * 16, dtype=torch.uint8)


def class_locations(label, value, u, count=None, index=None, workspace=None):
    assert label.dtype == torch.uint8 and label.is_contiguous() and u.dtype == torch.int32 and u.dim() == 1
    flat = label.reshape(-1).numpy()
    N, R, value = flat.size, u.numel(), int(value)
    assert N >= 1 and 1 <= R <= 1 << 20 and -1 <= value <= 255
    match = flat != 0 if value == -1 else flat == np.uint8(value)
    nchunks = (N + CHUNK - 1) // CHUNK
    padded = np.zeros(nchunks * CHUNK, bool)
    padded[:N] = match
    per_chunk = padded.reshape(nchunks, CHUNK).sum(axis=1).astype(np.uint32)
    prefix = (np.cumsum(per_chunk, dtype=np.uint64) - per_chunk).astype(np.uint32)
    total = int(per_chunk.sum(dtype=np.uint64))
    res = np.full(R, -1, np.int32)
    if total:
        rank = ((u.numpy().view(np.uint32).astype(np.uint64) * np.uint64(total)) >> np.uint64(32)).astype(np.uint32)
        chunk = np.searchsorted(prefix, rank, side="right") - 1
        for j in range(R):
            c = int(chunk[j])
            inside = np.flatnonzero(padded[c * CHUNK:(c + 1) * CHUNK])
            res[j] = c * CHUNK + int(inside[int(rank[j]) - int(prefix[c])])
    if count is None:
        count = torch.empty(1, dtype=torch.int64)
    if index is None:
        index = torch.empty(R, dtype=torch.int32)
    assert count.dtype == torch.int64 and count.numel() == 1 and index.dtype == torch.int32 and index.numel() == R
    count[0] = total
    index.copy_(torch.from_numpy(res))
    return count, index
