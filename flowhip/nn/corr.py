"""Correlation block: volume build + pyramid + per-iteration window lookup.

Reference behavior: core/corr.py (CorrBlock). The compute goes through
`flowhip.ops` so the HIP kernels (MFMA GEMM #1, pyramid #2, fused lookup #3)
run on GPU and the torch path on CPU. Unlike the reference, the window offset
grid lives on-device inside the lookup kernel (no per-iteration host->device
`delta` transfer — SURVEY.md §2.9 quirk 8), which also makes the iteration
loop hipGraph-capturable.
"""

from .. import ops
from ..ops.functional import AltOperandLevels, alt_f1_rows


class CorrBlock:
    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self.num_levels = num_levels
        self.radius = radius
        corr = ops.corr_volume(fmap1, fmap2)  # (B*H*W, 1, H, W)
        self.corr_pyramid = ops.corr_pyramid(corr, num_levels)

    def __call__(self, coords):
        out, self.corr_pyramid = ops.corr_lookup_chained(
            self.corr_pyramid, coords, self.radius)
        return out


class AlternateCorrBlock:
    """On-demand correlation (upstream RAFT's `--alternate_corr`): same call
    signature and output as CorrBlock, but the window correlations are
    computed from the two feature maps at every lookup, so nothing larger
    than O(P*D) is kept — no all-pairs volume, no pyramid of it. Per pair it
    builds the pooled f2 levels (and, on GPU, the bf16 f1 rows) once."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self.num_levels = num_levels
        self.radius = radius
        self.fmap1 = fmap1
        self.fmap2 = fmap2
        self.levels = ops.alt_corr_pyramid(fmap2, num_levels)
        self.f1_rows = None
        if isinstance(self.levels, AltOperandLevels):
            self.f1_rows = alt_f1_rows(fmap1)

    def __call__(self, coords):
        return ops.alt_corr_lookup(self.fmap1, self.levels, coords,
                                   self.radius, fmap2=self.fmap2,
                                   f1_rows=self.f1_rows)
