"""Which kernel did the gather-GEMM launches of a block of test code take?  A context manager around
hip_backend.profile_start() / profile_stop(layers=True): the shape tag of every profiled launch names its kernel in brackets
(hip_backend._gg_tag: the library's route queries, not a guess), so a test can assert the route it used to assume.

    with route_probe.launches() as seen:
        y = ops.fused_conv3d(...)
    assert seen.kernels("gather_gemm_bf16") == ["halo 4x8x16"]
"""
import contextlib
import re

from rehrseg_amd import hip_backend


class Launches(list):
    """(family, tag) of every profiled launch, in order."""

    def kernels(self, *families):
        """The bracketed kernel names of the launches of these profiling families (all gather-GEMM families by default)."""
        families = families or ("gather_gemm", "gather_gemm_bf16", "wino_conv", "wino22_conv")
        return [re.search(r"\[([^\]]*)\]$", tag).group(1) for fam, tag in self if fam in families]


@contextlib.contextmanager
def launches():
    seen = Launches()
    hip_backend.profile_start()
    try:
        yield seen
    finally:
        seen.extend((fam, tag) for fam, tag, _, _ in hip_backend.profile_stop(layers=True))
