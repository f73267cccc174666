"""The census of csrc/gemm.hip's compiled GEMM kernels: one row per instantiation of gemm_kernel / gemm_mixed_kernel /
gemm_pair_kernel that a valid descriptor reaches, with the smallest shapes that select it, and the helpers that run one case of
a row against float64 inside sentinel-guarded buffers (tests/test_gpu_gemm_census.py).  tests/test_lib_abi.py checks on the CPU
that the table is complete: dosx_gemm_kernel_name, swept over every family, names nothing that has no row here, and every row's
shapes still select the kernel the row names.  Plain data and helpers: nothing here is collected by pytest.

What "the right kernel ran" can mean here: the library reports its plan (dosx_gemm_kernel_name, dosx_gemm_partial_rows), not the
launch.  A tail split is recognised from (M, N, epilogue) alone and dosx_gemm_pair reports nothing, while both fall back to the
plain grid / to two launches when a precondition fails (alignment, stats_out / norm_out, a combination without a mixed kernel).
The tests therefore assert those preconditions on the real descriptors (vector staging, equal column tiles, no stats_out /
norm_out on a split row, a MIXED_ROWS form), and the LayerNorm-backward splits also show in their partial rows, which only the
split grid numbers through both parts; beyond that, which symbol the GPU executed is the profiler's to say."""
import ctypes as C
import math
import re

import numpy as np
import torch

TOL = 2e-5                       # (tests/gpu_util.TOL; restated so that the CPU-only completeness test needs no torch.cuda)
LN_EPS = 1e-5
BK = 32                          # k-chunk of gemm_body (csrc/gemm.hip: BK)
GEMM_KMAX = 1024                 # largest K of a LayerNorm prologue (csrc/gemm.hip: GEMM_KMAX)
TILE_ROWS = {0: 16, 1: 32, 2: 64, 3: 48}      # rows per workgroup by gemm_kernel's RT code
SENT_BITS = 0x7FC0BEEF           # sentinel of every output buffer: a NaN with a payload (an unwritten output is a NaN too)

# ---- families (dispatch_gemm): (w_layout, vector staging, prologues, epilogues) ---------------------------------------
FAMILIES = {
    "generic_nk": (0, 0, ("NONE",), ("BIAS_ACT",)),
    "generic_kn": (1, 0, ("NONE",), ("BIAS_ACT",)),
    "plain_nk": (0, 1, ("NONE", "PRELU", "LN_PRELU", "ROWLN"), ("BIAS_ACT",)),
    "ln": (0, 1, ("NONE",), ("LN",)),
    "plain_kn": (1, 1, ("NONE",), ("BIAS_ACT",)),
    "bwd": (1, 1, ("NONE",), ("PRELU_LN_BWD", "RELU_MASK", "ROWLN_BWD", "PRELU_BWD")),
    "segsum": (0, 1, ("LN_PRELU",), ("SEGSUM",)),
    "seg_bwd": (1, 1, ("NONE",), ("PRELU_LN_BWD_SEG",)),
}
SWEEP_N = (16, 64, 128, 132, 256, 260, 512, 1024)

# ---- error bounds ----------------------------------------------------------------------------------------------------
# Every output is compared per row, |got - ref64| / (largest |ref64| of that row), against TOL.  An output that cancels gets
# 4 x the error of the same formula in plain fp32 torch against float64 ON THE OPERANDS THE TEST USES (make_inputs on the
# device: its generator's stream is the device's, so a figure taken from CPU operands is about other numbers) where that
# exceeds TOL - never a figure of the kernel's.  Every row-wise output and every column sum stays at 0.6e-7 .. 1.4e-6 in fp32
# torch, the LayerNorm-backward rows included: TOL.  What cancels is the PReLU slope gradient, ONE scalar summed over all
# M x N signed terms and judged against its own magnitude; test_gpu_gemm_census prints its fp32-torch error for every case
# ("fp32 torch [epilogue]: dalpha ..."), and the largest of each epilogue over all census cases is:
# The two figures kept are cases where that sum happens to cancel almost to zero on the device's (seeded, reproducible: the same
# figure in every run) random stream, so fp32 torch itself is that far off there and 1e-6 or better elsewhere; a change of the
# seeds or of make_inputs moves them and they must be re-read from the test's printout.  The measure that does not depend on
# the stream, |error| / sum of |terms|, is held to TOL next to it (errors(): "dalpha/terms", worst measured 2.3e-8).
#   key: (epilogue, output)          4 x the fp32-torch baseline      (baseline, at M, N, K)
BOUNDS = {
    ("PRELU_LN_BWD", "dalpha"): 2.83e-4,                            # 7.07e-05 at 4097, 132, 160
    ("PRELU_LN_BWD_SEG", "dalpha"): 9.44e-5,                        # 2.36e-05 at 666, 100, 64 (two K-segments)
}                                                                   # (PRELU_BWD dalpha: 3.16e-06 at 4097, 128, 4 - TOL)


def bound(epi, what):
    return BOUNDS.get((epi, what), TOL)


# ---- gemm_kernel rows ----------------------------------------------------------------------------------------------------
# (family, prologue, epilogue, extra, kernel, (N that fills the column tiles, M, M'), (ragged N, M, M'))
#   M: the smallest row count (at that N) that selects the kernel and leaves exactly ONE row in the last row tile;
#   M': the next one whose last tile is one row short of full.  extra "stats": only stats_out / norm_out widen the plain
#   epilogue's column tile past 128.  Derived by scanning dosx_gemm_kernel_name; test_gemm_census_is_complete re-derives them.
ROWS = [
    ("generic_nk", "NONE", "BIAS_ACT", "", "gemm_kernel<0, 1, 0, 0, 0, 0>", (128, 17, 31), (100, 17, 31)),
    ("generic_nk", "NONE", "BIAS_ACT", "stats", "gemm_kernel<0, 2, 0, 0, 0, 0>", (256, 17, 31), (132, 17, 31)),
    ("generic_nk", "NONE", "BIAS_ACT", "stats", "gemm_kernel<0, 4, 0, 0, 0, 0>", (512, 17, 31), (260, 17, 31)),
    ("generic_nk", "NONE", "BIAS_ACT", "", "gemm_kernel<1, 1, 0, 0, 0, 0>", (128, 4097, 4127), (100, 4097, 4127)),
    ("generic_nk", "NONE", "BIAS_ACT", "stats", "gemm_kernel<1, 2, 0, 0, 0, 0>", (256, 2049, 2079), (132, 2049, 2079)),
    ("generic_nk", "NONE", "BIAS_ACT", "stats", "gemm_kernel<1, 4, 0, 0, 0, 0>", (512, 1025, 1055), (260, 1345, 1375)),
    ("generic_nk", "NONE", "BIAS_ACT", "", "gemm_kernel<2, 1, 0, 0, 0, 0>", (256, 4097, 4159), (228, 4097, 4159)),
    ("generic_nk", "NONE", "BIAS_ACT", "stats", "gemm_kernel<2, 2, 0, 0, 0, 0>", (256, 4097, 4159), (132, 4097, 4159)),
    ("generic_nk", "NONE", "BIAS_ACT", "", "gemm_kernel<3, 1, 0, 0, 0, 0>", (128, 8209, 8207), (100, 8209, 8207)),
    ("generic_kn", "NONE", "BIAS_ACT", "", "gemm_kernel<0, 1, 1, 0, 0, 0>", (128, 17, 31), (100, 17, 31)),
    ("generic_kn", "NONE", "BIAS_ACT", "stats", "gemm_kernel<0, 2, 1, 0, 0, 0>", (256, 17, 31), (132, 17, 31)),
    ("generic_kn", "NONE", "BIAS_ACT", "stats", "gemm_kernel<0, 4, 1, 0, 0, 0>", (512, 17, 31), (260, 17, 31)),
    ("generic_kn", "NONE", "BIAS_ACT", "", "gemm_kernel<1, 1, 1, 0, 0, 0>", (128, 4097, 4127), (100, 4097, 4127)),
    ("generic_kn", "NONE", "BIAS_ACT", "stats", "gemm_kernel<1, 2, 1, 0, 0, 0>", (256, 2049, 2079), (132, 2049, 2079)),
    ("generic_kn", "NONE", "BIAS_ACT", "stats", "gemm_kernel<1, 4, 1, 0, 0, 0>", (512, 1025, 1055), (260, 1345, 1375)),
    ("generic_kn", "NONE", "BIAS_ACT", "", "gemm_kernel<2, 1, 1, 0, 0, 0>", (256, 4097, 4159), (228, 4097, 4159)),
    ("generic_kn", "NONE", "BIAS_ACT", "stats", "gemm_kernel<2, 2, 1, 0, 0, 0>", (256, 4097, 4159), (132, 4097, 4159)),
    ("generic_kn", "NONE", "BIAS_ACT", "", "gemm_kernel<3, 1, 1, 0, 0, 0>", (128, 8209, 8207), (100, 8209, 8207)),
    ("plain_nk", "NONE", "BIAS_ACT", "", "gemm_kernel<0, 1, 0, 0, 1, 0>", (128, 17, 31), (100, 17, 31)),
    ("plain_nk", "NONE", "BIAS_ACT", "stats", "gemm_kernel<0, 2, 0, 0, 1, 0>", (256, 17, 31), (132, 17, 31)),
    ("plain_nk", "NONE", "BIAS_ACT", "stats", "gemm_kernel<0, 4, 0, 0, 1, 0>", (512, 17, 31), (260, 17, 31)),
    ("plain_nk", "NONE", "BIAS_ACT", "", "gemm_kernel<1, 1, 0, 0, 1, 0>", (128, 4097, 4127), (100, 4097, 4127)),
    ("plain_nk", "NONE", "BIAS_ACT", "stats", "gemm_kernel<1, 2, 0, 0, 1, 0>", (256, 2049, 2079), (132, 2049, 2079)),
    ("plain_nk", "NONE", "BIAS_ACT", "stats", "gemm_kernel<1, 4, 0, 0, 1, 0>", (512, 1025, 1055), (260, 1345, 1375)),
    ("plain_nk", "NONE", "BIAS_ACT", "", "gemm_kernel<2, 1, 0, 0, 1, 0>", (256, 4097, 4159), (228, 4097, 4159)),
    ("plain_nk", "NONE", "BIAS_ACT", "stats", "gemm_kernel<2, 2, 0, 0, 1, 0>", (256, 4097, 4159), (132, 4097, 4159)),
    ("plain_nk", "NONE", "BIAS_ACT", "", "gemm_kernel<3, 1, 0, 0, 1, 0>", (128, 8209, 8207), (100, 8209, 8207)),
    ("plain_nk", "PRELU", "BIAS_ACT", "", "gemm_kernel<0, 1, 0, 1, 1, 0>", (128, 17, 31), (100, 17, 31)),
    ("plain_nk", "PRELU", "BIAS_ACT", "stats", "gemm_kernel<0, 2, 0, 1, 1, 0>", (256, 17, 31), (132, 17, 31)),
    ("plain_nk", "PRELU", "BIAS_ACT", "stats", "gemm_kernel<0, 4, 0, 1, 1, 0>", (512, 17, 31), (260, 17, 31)),
    ("plain_nk", "PRELU", "BIAS_ACT", "", "gemm_kernel<1, 1, 0, 1, 1, 0>", (128, 4097, 4127), (100, 4097, 4127)),
    ("plain_nk", "PRELU", "BIAS_ACT", "stats", "gemm_kernel<1, 2, 0, 1, 1, 0>", (256, 2049, 2079), (132, 2049, 2079)),
    ("plain_nk", "PRELU", "BIAS_ACT", "stats", "gemm_kernel<1, 4, 0, 1, 1, 0>", (512, 1025, 1055), (260, 1345, 1375)),
    ("plain_nk", "PRELU", "BIAS_ACT", "", "gemm_kernel<2, 1, 0, 1, 1, 0>", (256, 4097, 4159), (228, 4097, 4159)),
    ("plain_nk", "PRELU", "BIAS_ACT", "stats", "gemm_kernel<2, 2, 0, 1, 1, 0>", (256, 4097, 4159), (132, 4097, 4159)),
    ("plain_nk", "PRELU", "BIAS_ACT", "", "gemm_kernel<3, 1, 0, 1, 1, 0>", (128, 8209, 8207), (100, 8209, 8207)),
    ("plain_nk", "LN_PRELU", "BIAS_ACT", "", "gemm_kernel<0, 1, 0, 2, 1, 0>", (128, 17, 31), (100, 17, 31)),
    ("plain_nk", "LN_PRELU", "BIAS_ACT", "stats", "gemm_kernel<0, 2, 0, 2, 1, 0>", (256, 17, 31), (132, 17, 31)),
    ("plain_nk", "LN_PRELU", "BIAS_ACT", "", "gemm_kernel<1, 1, 0, 2, 1, 0>", (128, 4097, 4127), (100, 4097, 4127)),
    ("plain_nk", "LN_PRELU", "BIAS_ACT", "stats", "gemm_kernel<1, 2, 0, 2, 1, 0>", (256, 2049, 2079), (132, 2049, 2079)),
    ("plain_nk", "LN_PRELU", "BIAS_ACT", "", "gemm_kernel<2, 1, 0, 2, 1, 0>", (256, 4097, 4159), (228, 4097, 4159)),
    ("plain_nk", "LN_PRELU", "BIAS_ACT", "stats", "gemm_kernel<2, 2, 0, 2, 1, 0>", (256, 4097, 4159), (132, 4097, 4159)),
    ("plain_nk", "LN_PRELU", "BIAS_ACT", "", "gemm_kernel<3, 1, 0, 2, 1, 0>", (128, 8209, 8207), (100, 8209, 8207)),
    ("plain_nk", "ROWLN", "BIAS_ACT", "", "gemm_kernel<0, 1, 0, 3, 1, 0>", (128, 17, 31), (100, 17, 31)),
    ("plain_nk", "ROWLN", "BIAS_ACT", "stats", "gemm_kernel<0, 2, 0, 3, 1, 0>", (256, 17, 31), (132, 17, 31)),
    ("plain_nk", "ROWLN", "BIAS_ACT", "", "gemm_kernel<1, 1, 0, 3, 1, 0>", (128, 4097, 4127), (100, 4097, 4127)),
    ("plain_nk", "ROWLN", "BIAS_ACT", "stats", "gemm_kernel<1, 2, 0, 3, 1, 0>", (256, 2049, 2079), (132, 2049, 2079)),
    ("plain_nk", "ROWLN", "BIAS_ACT", "", "gemm_kernel<2, 1, 0, 3, 1, 0>", (256, 4097, 4159), (228, 4097, 4159)),
    ("plain_nk", "ROWLN", "BIAS_ACT", "stats", "gemm_kernel<2, 2, 0, 3, 1, 0>", (256, 4097, 4159), (132, 4097, 4159)),
    ("plain_nk", "ROWLN", "BIAS_ACT", "", "gemm_kernel<3, 1, 0, 3, 1, 0>", (128, 8209, 8207), (100, 8209, 8207)),
    ("ln", "NONE", "LN", "", "gemm_kernel<0, 1, 0, 0, 1, 1>", (128, 17, 31), (100, 17, 31)),
    ("ln", "NONE", "LN", "", "gemm_kernel<0, 2, 0, 0, 1, 1>", (256, 17, 31), (132, 17, 31)),
    ("ln", "NONE", "LN", "", "gemm_kernel<0, 4, 0, 0, 1, 1>", (512, 17, 31), (260, 17, 31)),
    ("ln", "NONE", "LN", "", "gemm_kernel<1, 1, 0, 0, 1, 1>", (128, 4097, 4127), (100, 4097, 4127)),
    ("ln", "NONE", "LN", "", "gemm_kernel<1, 2, 0, 0, 1, 1>", (256, 4097, 4127), (132, 4097, 4127)),
    ("ln", "NONE", "LN", "", "gemm_kernel<1, 4, 0, 0, 1, 1>", (512, 4097, 4127), (260, 4097, 4127)),
    ("ln", "NONE", "LN", "", "gemm_kernel<2, 1, 0, 0, 1, 1>", (128, 12289, 12351), (100, 12289, 12351)),
    ("ln", "NONE", "LN", "", "gemm_kernel<2, 2, 0, 0, 1, 1>", (256, 12289, 12351), (132, 12289, 12351)),
    ("ln", "NONE", "LN", "", "gemm_kernel<3, 1, 0, 0, 1, 1>", (128, 8209, 8207), (100, 8209, 8207)),
    ("ln", "NONE", "LN", "", "gemm_kernel<3, 2, 0, 0, 1, 1>", (256, 8209, 8207), (132, 8209, 8207)),
    ("plain_kn", "NONE", "BIAS_ACT", "", "gemm_kernel<0, 1, 1, 0, 1, 0>", (128, 17, 31), (100, 17, 31)),
    ("plain_kn", "NONE", "BIAS_ACT", "stats", "gemm_kernel<0, 2, 1, 0, 1, 0>", (256, 17, 31), (132, 17, 31)),
    ("plain_kn", "NONE", "BIAS_ACT", "stats", "gemm_kernel<0, 4, 1, 0, 1, 0>", (512, 17, 31), (260, 17, 31)),
    ("plain_kn", "NONE", "BIAS_ACT", "", "gemm_kernel<1, 1, 1, 0, 1, 0>", (128, 4097, 4127), (100, 4097, 4127)),
    ("plain_kn", "NONE", "BIAS_ACT", "stats", "gemm_kernel<1, 2, 1, 0, 1, 0>", (256, 2049, 2079), (132, 2049, 2079)),
    ("plain_kn", "NONE", "BIAS_ACT", "stats", "gemm_kernel<1, 4, 1, 0, 1, 0>", (512, 1025, 1055), (260, 1345, 1375)),
    ("plain_kn", "NONE", "BIAS_ACT", "", "gemm_kernel<2, 1, 1, 0, 1, 0>", (256, 4097, 4159), (228, 4097, 4159)),
    ("plain_kn", "NONE", "BIAS_ACT", "stats", "gemm_kernel<2, 2, 1, 0, 1, 0>", (256, 4097, 4159), (132, 4097, 4159)),
    ("plain_kn", "NONE", "BIAS_ACT", "", "gemm_kernel<3, 1, 1, 0, 1, 0>", (128, 8209, 8207), (100, 8209, 8207)),
    ("bwd", "NONE", "PRELU_LN_BWD", "", "gemm_kernel<0, 1, 1, 0, 1, 2>", (128, 17, 31), (100, 17, 31)),
    ("bwd", "NONE", "PRELU_LN_BWD", "", "gemm_kernel<0, 2, 1, 0, 1, 2>", (256, 17, 31), (132, 17, 31)),
    ("bwd", "NONE", "PRELU_LN_BWD", "", "gemm_kernel<0, 4, 1, 0, 1, 2>", (512, 17, 31), (260, 17, 31)),
    ("bwd", "NONE", "PRELU_LN_BWD", "", "gemm_kernel<1, 1, 1, 0, 1, 2>", (128, 4097, 4127), (100, 4097, 4127)),
    ("bwd", "NONE", "PRELU_LN_BWD", "", "gemm_kernel<1, 2, 1, 0, 1, 2>", (256, 4097, 4127), (132, 4097, 4127)),
    ("bwd", "NONE", "PRELU_LN_BWD", "", "gemm_kernel<1, 4, 1, 0, 1, 2>", (512, 4097, 4127), (260, 4097, 4127)),
    ("bwd", "NONE", "PRELU_LN_BWD", "", "gemm_kernel<2, 1, 1, 0, 1, 2>", (128, 12289, 12351), (100, 12289, 12351)),
    ("bwd", "NONE", "PRELU_LN_BWD", "", "gemm_kernel<2, 2, 1, 0, 1, 2>", (256, 12289, 12351), (132, 12289, 12351)),
    ("bwd", "NONE", "PRELU_LN_BWD", "", "gemm_kernel<3, 1, 1, 0, 1, 2>", (128, 8209, 8207), (100, 8209, 8207)),
    ("bwd", "NONE", "PRELU_LN_BWD", "", "gemm_kernel<3, 2, 1, 0, 1, 2>", (256, 8209, 8207), (132, 8209, 8207)),
    ("bwd", "NONE", "RELU_MASK", "", "gemm_kernel<0, 1, 1, 0, 1, 3>", (128, 17, 31), (100, 17, 31)),
    ("bwd", "NONE", "RELU_MASK", "", "gemm_kernel<1, 1, 1, 0, 1, 3>", (128, 4097, 4127), (100, 4097, 4127)),
    ("bwd", "NONE", "RELU_MASK", "", "gemm_kernel<2, 1, 1, 0, 1, 3>", (256, 4097, 4159), (228, 4097, 4159)),
    ("bwd", "NONE", "RELU_MASK", "", "gemm_kernel<3, 1, 1, 0, 1, 3>", (128, 8209, 8207), (100, 8209, 8207)),
    ("bwd", "NONE", "ROWLN_BWD", "", "gemm_kernel<0, 1, 1, 0, 1, 4>", (128, 17, 31), (100, 17, 31)),
    ("bwd", "NONE", "ROWLN_BWD", "", "gemm_kernel<0, 2, 1, 0, 1, 4>", (256, 17, 31), (132, 17, 31)),
    ("bwd", "NONE", "ROWLN_BWD", "", "gemm_kernel<0, 4, 1, 0, 1, 4>", (512, 17, 31), (260, 17, 31)),
    ("bwd", "NONE", "ROWLN_BWD", "", "gemm_kernel<1, 1, 1, 0, 1, 4>", (128, 4097, 4127), (100, 4097, 4127)),
    ("bwd", "NONE", "ROWLN_BWD", "", "gemm_kernel<1, 2, 1, 0, 1, 4>", (256, 4097, 4127), (132, 4097, 4127)),
    ("bwd", "NONE", "ROWLN_BWD", "", "gemm_kernel<1, 4, 1, 0, 1, 4>", (512, 4097, 4127), (260, 4097, 4127)),
    ("bwd", "NONE", "ROWLN_BWD", "", "gemm_kernel<2, 1, 1, 0, 1, 4>", (128, 12289, 12351), (100, 12289, 12351)),
    ("bwd", "NONE", "ROWLN_BWD", "", "gemm_kernel<2, 2, 1, 0, 1, 4>", (256, 12289, 12351), (132, 12289, 12351)),
    ("bwd", "NONE", "ROWLN_BWD", "", "gemm_kernel<3, 1, 1, 0, 1, 4>", (128, 8209, 8207), (100, 8209, 8207)),
    ("bwd", "NONE", "ROWLN_BWD", "", "gemm_kernel<3, 2, 1, 0, 1, 4>", (256, 8209, 8207), (132, 8209, 8207)),
    ("bwd", "NONE", "PRELU_BWD", "", "gemm_kernel<0, 1, 1, 0, 1, 5>", (128, 17, 31), (100, 17, 31)),
    ("bwd", "NONE", "PRELU_BWD", "", "gemm_kernel<1, 1, 1, 0, 1, 5>", (128, 4097, 4127), (100, 4097, 4127)),
    ("bwd", "NONE", "PRELU_BWD", "", "gemm_kernel<2, 1, 1, 0, 1, 5>", (256, 4097, 4159), (228, 4097, 4159)),
    ("bwd", "NONE", "PRELU_BWD", "", "gemm_kernel<3, 1, 1, 0, 1, 5>", (128, 8209, 8207), (100, 8209, 8207)),
]

# node-aligned tiles (one workgroup per tile of a destination-sorted graph, 48 rows at most): (family, pro, epi, kernel, N, ragged N)
SEG_ROWS = [
    ("segsum", "LN_PRELU", "SEGSUM", "gemm_kernel<3, 1, 0, 2, 1, 6>", 128, 100),
    ("segsum", "LN_PRELU", "SEGSUM", "gemm_kernel<3, 2, 0, 2, 1, 6>", 256, 132),
    ("seg_bwd", "NONE", "PRELU_LN_BWD_SEG", "gemm_kernel<3, 1, 1, 0, 1, 7>", 128, 100),
    ("seg_bwd", "NONE", "PRELU_LN_BWD_SEG", "gemm_kernel<3, 2, 1, 0, 1, 7>", 256, 132),
]

# Names the sweep produces that no valid call launches: (family, pro, epi, extra, kernel, M, N, what refuses it)
REFUSED = [
    # a 512-column tile + the LayerNorm prologue's gamma / beta exceed the 160 KB of LDS: launch_gemm3 refuses
    ("plain_nk", "LN_PRELU", "BIAS_ACT", "stats", "gemm_kernel<0, 4, 0, 2, 1, 0>", 17, 512, "exceeds the 160 KB LDS"),
    ("plain_nk", "LN_PRELU", "BIAS_ACT", "stats", "gemm_kernel<1, 4, 0, 2, 1, 0>", 1025, 512, "exceeds the 160 KB LDS"),
    ("plain_nk", "ROWLN", "BIAS_ACT", "stats", "gemm_kernel<0, 4, 0, 3, 1, 0>", 17, 512, "exceeds the 160 KB LDS"),
    ("plain_nk", "ROWLN", "BIAS_ACT", "stats", "gemm_kernel<1, 4, 0, 3, 1, 0>", 1025, 512, "exceeds the 160 KB LDS"),
    # stats_out widens the column tile of ANY epilogue in gemm_plan, but only the plain one writes it: gemm_validate refuses
    ("bwd", "NONE", "RELU_MASK", "stats", "gemm_kernel<0, 2, 1, 0, 1, 3>", 17, 256, "stats_out needs the plain epilogue"),
    ("bwd", "NONE", "RELU_MASK", "stats", "gemm_kernel<0, 4, 1, 0, 1, 3>", 17, 512, "stats_out needs the plain epilogue"),
    ("bwd", "NONE", "RELU_MASK", "stats", "gemm_kernel<1, 2, 1, 0, 1, 3>", 2049, 256, "stats_out needs the plain epilogue"),
    ("bwd", "NONE", "RELU_MASK", "stats", "gemm_kernel<1, 4, 1, 0, 1, 3>", 1025, 512, "stats_out needs the plain epilogue"),
    ("bwd", "NONE", "RELU_MASK", "stats", "gemm_kernel<2, 2, 1, 0, 1, 3>", 4097, 256, "stats_out needs the plain epilogue"),
    ("bwd", "NONE", "PRELU_BWD", "stats", "gemm_kernel<0, 2, 1, 0, 1, 5>", 17, 256, "stats_out needs the plain epilogue"),
    ("bwd", "NONE", "PRELU_BWD", "stats", "gemm_kernel<0, 4, 1, 0, 1, 5>", 17, 512, "stats_out needs the plain epilogue"),
    ("bwd", "NONE", "PRELU_BWD", "stats", "gemm_kernel<1, 2, 1, 0, 1, 5>", 2049, 256, "stats_out needs the plain epilogue"),
    ("bwd", "NONE", "PRELU_BWD", "stats", "gemm_kernel<1, 4, 1, 0, 1, 5>", 1025, 512, "stats_out needs the plain epilogue"),
    ("bwd", "NONE", "PRELU_BWD", "stats", "gemm_kernel<2, 2, 1, 0, 1, 5>", 4097, 256, "stats_out needs the plain epilogue"),
]

# ---- the tail split (gemm_tail_split -> gemm_mixed_kernel<RTA, RTB, NTW, WL, PRO, 1, EPI>) -----------------------------------
# dosx_gemm_kernel_name names the HEAD tile only; the split shows in dosx_gemm_partial_rows(M, N, epi), which then differs from
# ceil(M / head tile rows).  (family, pro, epi, mixed kernel, head kernel as named, (N, M, M', partial rows of M, of M'), (ragged ...))
#   M, M': the smallest split row counts whose last TAIL tile holds one row / is one row short
MIXED_ROWS = [
    ("plain_nk", "NONE", "BIAS_ACT", "gemm_mixed_kernel<2, 1, 1, 0, 0, 1, 0>", "gemm_kernel<2, 1, 0, 0, 1, 0>",
     (512, 4129, 4159, 66, 66), (484, 4129, 4159, 66, 66)),
    ("plain_nk", "ROWLN", "BIAS_ACT", "gemm_mixed_kernel<2, 1, 1, 0, 3, 1, 0>", "gemm_kernel<2, 1, 0, 3, 1, 0>",
     (512, 4129, 4159, 66, 66), (484, 4129, 4159, 66, 66)),
    ("plain_kn", "NONE", "BIAS_ACT", "gemm_mixed_kernel<2, 1, 1, 1, 0, 1, 0>", "gemm_kernel<2, 1, 1, 0, 1, 0>",
     (512, 4129, 4159, 66, 66), (484, 4129, 4159, 66, 66)),
    ("bwd", "NONE", "RELU_MASK", "gemm_mixed_kernel<2, 1, 1, 1, 0, 1, 3>", "gemm_kernel<2, 1, 1, 0, 1, 3>",
     (512, 4129, 4159, 66, 66), (484, 4129, 4159, 66, 66)),
    ("bwd", "NONE", "ROWLN_BWD", "gemm_mixed_kernel<2, 1, 2, 1, 0, 1, 4>", "gemm_kernel<2, 2, 1, 0, 1, 4>",
     (256, 16417, 16447, 258, 258), (132, 16417, 16447, 258, 258)),
    ("bwd", "NONE", "ROWLN_BWD", "gemm_mixed_kernel<2, 3, 2, 1, 0, 1, 4>", "gemm_kernel<2, 2, 1, 0, 1, 4>",
     (256, 24593, 24591, 428, 427), (132, 24593, 24591, 428, 427)),
    ("ln", "NONE", "LN", "gemm_mixed_kernel<1, 0, 4, 0, 0, 1, 1>", "gemm_kernel<1, 4, 0, 0, 1, 1>",
     (512, 8209, 8223, 258, 258), (260, 8209, 8223, 258, 258)),
    ("bwd", "NONE", "PRELU_LN_BWD", "gemm_mixed_kernel<1, 0, 4, 1, 0, 1, 2>", "gemm_kernel<1, 4, 1, 0, 1, 2>",
     (512, 8209, 8223, 258, 258), (260, 8209, 8223, 258, 258)),
]

# ---- dosx_gemm_pair ------------------------------------------------------------------------------------------------------------
# gemm_pair_kernel<RT, NTW>: plain W[N,K] problems of one N; the tile height is that of ONE problem with all the rows, so the
# kernel is named by dosx_gemm_kernel_name at M1 + M2.  NTW = 2 needs norm_out (or stats_out) on both; with it the policy counts
# two 128-column tiles, so the 48-row height (one column tile only) never pairs: gemm_pair_kernel<3, 2> is unreachable.
#   (kernel, head kernel named at M1 + M2, extra, N, ragged N, M1, M2)
PAIR_ROWS = [
    ("gemm_pair_kernel<0, 1>", "gemm_kernel<0, 1, 0, 0, 1, 0>", "", 128, 100, 17, 31),
    ("gemm_pair_kernel<1, 1>", "gemm_kernel<1, 1, 0, 0, 1, 0>", "", 128, 100, 33, 4095),
    ("gemm_pair_kernel<3, 1>", "gemm_kernel<3, 1, 0, 0, 1, 0>", "", 128, 100, 4129, 4079),
    ("gemm_pair_kernel<2, 1>", "gemm_kernel<2, 1, 0, 0, 1, 0>", "", 128, 100, 6209, 6143),
    ("gemm_pair_kernel<0, 2>", "gemm_kernel<0, 2, 0, 0, 1, 0>", "norm", 256, 132, 17, 31),
    ("gemm_pair_kernel<1, 2>", "gemm_kernel<1, 2, 0, 0, 1, 0>", "norm", 256, 132, 33, 2047),
    ("gemm_pair_kernel<2, 2>", "gemm_kernel<2, 2, 0, 0, 1, 0>", "norm", 256, 132, 3137, 3007),
]
# the two encoders' backward products at their own tile heights in one grid: 16-row tiles (M1) + 48-row tiles (M2), N = 128 only
PAIR_MIXED = ("gemm_mixed_kernel<0, 3, 1, 1, 0, 1, 5>", "gemm_kernel<0, 1, 1, 0, 1, 5>", "gemm_kernel<3, 1, 1, 0, 1, 5>", 128, 33, 8209)


def n_instantiations():
    return len(ROWS) + len(SEG_ROWS) + len(MIXED_ROWS) + len(PAIR_ROWS) + 1


# ---- host side: what dosx_gemm_kernel_name says (no GPU) ----------------------------------------------------------------------
def fake_desc(M, N, K, family, pro, epi, extra=""):
    """A descriptor with made-up (never dereferenced) addresses, as tests/test_lib_abi.py builds them.  The generic families
    get an A row stride that is no multiple of 4 floats: that is what takes the vector staging path away."""
    from dostransformer_amd import _abi, _lib
    wl, vec = FAMILIES[family][:2]
    g = _lib.Gemm()
    g.M, g.N, g.K, g.nseg, g.w_layout = M, N, K, 1, wl
    g.pro, g.epi = getattr(_abi, "DOSX_PRO_" + pro), getattr(_abi, "DOSX_EPI_" + epi)
    g.a[0].ld, g.a[0].width, g.ldw = (K if vec else K + 1), K, (K if wl == 0 else N)
    for f in {"": (), "stats": ("stats_out",), "norm": ("norm_out",)}[extra]:
        setattr(g, f, 0x10000)
    return g


def kernel_name(lib, g):
    buf = C.create_string_buffer(96)
    assert lib.dosx_gemm_kernel_name(C.byref(g), buf, 96) == 0
    return buf.value.decode()


def tile_rows(kernel):
    """Rows per workgroup of a gemm_kernel<RT, ...> name."""
    return TILE_ROWS[int(re.match(r"gemm_kernel<(\d)", kernel).group(1))]


def is_split(lib, M, N, epi, kernel):
    """dosx_gemm_kernel_name does not report a tail split; dosx_gemm_partial_rows does: one partial row per workgroup of ONE
    column tile (PRELU_BWD: per 128 columns), so a split call has another count than ceil(M / rows of the tile named)."""
    from dostransformer_amd import _abi
    e = getattr(_abi, "DOSX_EPI_" + epi)
    rows = lib.dosx_gemm_partial_rows(M, N, e)
    if epi == "PRELU_BWD":
        rows //= (N + 127) // 128
    return rows != (M + tile_rows(kernel) - 1) // tile_rows(kernel)


# ---- GPU side: one case = one launch inside guarded buffers against float64 -----------------------------------------------
def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, device=g.device, dtype=torch.float32) * scale


class Padded:
    """An input operand as a view into a larger NaN-filled buffer: one row above, 64 below, `left` / `right` columns."""

    def __init__(self, t, left=4, right=4, top=1, bottom=64):
        t = t if t.dim() == 2 else t[:, None]
        self.buf = torch.full((top + t.shape[0] + bottom, left + t.shape[1] + right), float("nan"), device=t.device, dtype=t.dtype)
        self.view = self.buf[top:top + t.shape[0], left:left + t.shape[1]]
        self.view.copy_(t)


class Guarded:
    """An output as a view into a larger sentinel-filled buffer (the bit pattern SENT_BITS everywhere, the view included): one
    guard row above, 64 below, `left` / `right` guard columns.  `allow` narrows what may be written inside the view."""

    def __init__(self, rows, cols, dev, left=4, right=4, top=1, bottom=64):
        self.bits = torch.full((top + rows + bottom, left + cols + right), SENT_BITS, device=dev, dtype=torch.int32)
        self.view = self.bits.view(torch.float32)[top:top + rows, left:left + cols]
        self.inside = torch.zeros_like(self.bits, dtype=torch.bool)
        self.inside[top:top + rows, left:left + cols] = True
        self._box = (top, rows, left, cols)

    def allow(self, cols_mask):
        top, rows, left, cols = self._box
        self.inside[top:top + rows, left:left + cols] = cols_mask[None, :]

    def intact(self):
        return bool((self.bits[~self.inside] == SENT_BITS).all())


def seg_graph(dev, seed):
    """A destination-sorted graph from tests/gpu_util._graph with a 60-in-degree node (two chunk tiles) and a 96-in-degree one,
    then - as a ghost-padded batch has them - a tile slot without rows that owns two ghost nodes and a slot that owns nothing."""
    from tests.gpu_util import _graph
    n = 40
    src, dst, rp, deg, tiles, E = _graph(n, seed, fat=(60, 96))
    t = tiles.cpu().numpy()
    eb, nb, pi = [list(r) for r in t]
    tiles = np.stack([np.asarray(eb + [E, E], np.int32), np.asarray(nb + [n + 2, n + 2], np.int32), np.asarray(pi[:-1] + [0, 0, 0], np.int32)])
    rp = torch.cat([rp, torch.full((2,), E, dtype=torch.int32, device=rp.device)])
    deg = np.concatenate([deg, [0, 0]])
    assert (np.diff(eb) > 48).sum() == 0 and int(deg.max()) > 48 and (np.diff(tiles[0]) == 0).sum() >= 2
    return dict(n=n + 2, E=E, src=src.to(dev), dst=dst.to(dev), rowptr=rp.to(dev), deg=deg, tiles=torch.from_numpy(tiles).to(dev))


def make_inputs(spec, dev):
    """The fp32 operands of one case, exactly as large as the formula needs (run() pads them).  Row magnitudes of A span
    10^-1.5 .. 10^1.5, so that a wrong small row shows against its own size."""
    M, N, K, wl, pro, epi = spec["M"], spec["N"], spec["K"], spec["wl"], spec["pro"], spec["epi"]
    g = _gen(dev, spec.get("seed", 0) + 7 * M + 3 * N + K)
    t = {}
    rowscale = torch.logspace(-1.5, 1.5, 7, device=dev)[torch.arange(M, device=dev) % 7][:, None]
    k1 = spec.get("k1", 0)                       # two K-segments: the first one gathered from a table through an index
    if k1:
        nx = 37
        t["x"] = _randn(g, nx, k1)
        t["idx"] = torch.randint(0, nx, (M,), generator=g, device=dev, dtype=torch.int32)
        t["a1"] = _randn(g, M, K - k1) * rowscale
    else:
        t["a"] = _randn(g, M, K) * rowscale
    if pro in ("PRELU", "LN_PRELU"):
        t["pro_alpha"] = torch.tensor([0.25], device=dev)
    if pro in ("LN_PRELU", "ROWLN"):
        t["pro_gamma"], t["pro_beta"] = 1 + 0.3 * _randn(g, K), 0.3 * _randn(g, K)
    if pro == "ROWLN":
        a = cat_a(t, torch.float64)
        mu = a.mean(1)
        t["pro_stats"] = torch.stack([mu, 1 / torch.sqrt(a.var(1, unbiased=False) + LN_EPS)], 1).float().contiguous()
    t["w"] = _randn(g, *((N, K) if wl == 0 else (K, N)), scale=K ** -0.5)
    if spec.get("bias"):
        t["bias"] = _randn(g, N)
    if spec.get("res"):
        t["res"] = _randn(g, M, N - spec.get("res_col0", 0))
    if spec.get("add"):
        t["add_pq"] = _randn(g, 29, 2 * N)
        t["add_ip"] = torch.randint(0, 29, (M,), generator=g, device=dev, dtype=torch.int32)
        t["add_iq"] = torch.randint(0, 29, (M,), generator=g, device=dev, dtype=torch.int32)
    if epi in ("PRELU_LN_BWD", "PRELU_LN_BWD_SEG"):
        t["epi_gamma"] = (0.5 + _randn(g, N).abs()) * torch.where(_randn(g, N) >= 0, 1.0, -1.0)
        t["epi_beta"], t["epi_alpha"] = 0.3 * _randn(g, N), torch.tensor([0.25], device=dev)
        xh = _randn(g, M, N).double()
        # y = xhat * gamma + beta stays 1e-3 or more away from the PReLU kink: closer, fp32 and float64 may rightly take
        # different branches of a discontinuous derivative
        y = xh * t["epi_gamma"].double() + t["epi_beta"].double()
        t["aux"] = torch.where(y.abs() < 1e-3, xh + 0.01 / t["epi_gamma"].double(), xh).float()
        t["aux_stats"] = _randn(g, M).abs() + 0.5
    elif epi == "ROWLN_BWD":
        t["epi_gamma"] = 1 + 0.3 * _randn(g, N)
        t["aux"] = _randn(g, M, N) * rowscale + _randn(g, M, 1)
        x = t["aux"].double()
        t["aux_stats"] = torch.stack([x.mean(1), 1 / torch.sqrt(x.var(1, unbiased=False) + LN_EPS)], 1).float().contiguous()
    elif epi in ("RELU_MASK", "PRELU_BWD"):
        t["aux"] = _randn(g, M, N)
        if epi == "PRELU_BWD":
            t["epi_alpha"] = torch.tensor([0.2], device=dev)
    if "graph" in spec:
        gr = spec["graph"]
        if spec.get("mean"):
            t["seg_scale"] = torch.from_numpy((1.0 / np.maximum(gr["deg"], 1)).astype(np.float32)).to(dev)
    return t


def cat_a(t, dt):
    if "a" in t:
        return t["a"].to(dt)
    return torch.cat([t["x"].to(dt)[t["idx"].long()], t["a1"].to(dt)], 1)


def _prelu(x, a):
    return torch.where(x >= 0, x, a * x)


def reference(spec, t, dt=torch.float64):
    """The formula of include/dosx.h for this descriptor in plain torch at precision `dt` on the fp32 operands."""
    N, wl, pro, epi = spec["N"], spec["wl"], spec["pro"], spec["epi"]
    c = lambda k: t[k].to(dt) if k in t else None
    a = cat_a(t, dt)
    if pro == "PRELU":
        a = _prelu(a, c("pro_alpha"))
    elif pro == "LN_PRELU":
        a = _prelu(a * c("pro_gamma") + c("pro_beta"), c("pro_alpha"))
    elif pro == "ROWLN":
        st = c("pro_stats")
        a = (a - st[:, :1]) * st[:, 1:] * c("pro_gamma") + c("pro_beta")
    acc = a @ (c("w").T if wl == 0 else c("w"))
    out = {}

    def ln_stats(y):
        mean = y.mean(1, keepdim=True)
        return mean, 1 / torch.sqrt(((y - mean) ** 2).mean(1, keepdim=True) + LN_EPS)

    def ln_bwd(dy, xh, gam, rstd):
        dxh = dy * gam
        return rstd * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))

    def seg_sum(rows):
        gr = spec["graph"]
        agg = torch.zeros(gr["n"], N, dtype=dt, device=rows.device).index_add_(0, gr["dst"].long(), rows)
        return agg * c("seg_scale")[:, None] if "seg_scale" in t else agg

    if epi == "BIAS_ACT":
        z = acc + c("bias") if "bias" in t else acc
        if spec.get("res_pre"):
            z = z + c("res")
        y = {0: z, 1: torch.relu(z), 2: torch.where(z >= 0, z, spec.get("slope", 0.01) * z)}[spec.get("act", 0)]
        if "res" in t and not spec.get("res_pre"):
            y = y.clone()
            y[:, spec.get("res_col0", 0):] += c("res")
        out["out"] = y
        if spec.get("stats") or spec.get("norm"):
            mean, rstd = ln_stats(y)
            if spec.get("stats"):
                out["stats_mean"], out["stats_rstd"] = mean, rstd
            if spec.get("norm"):
                out["norm"], out["norm_rstd"] = (y - mean) * rstd, rstd
    elif epi == "LN":
        z = acc + c("bias") if "bias" in t else acc
        if "add_pq" in t:
            pq = c("add_pq")
            z = z + pq[:, :N][t["add_ip"].long()] + pq[:, N:][t["add_iq"].long()]
        mean, rstd = ln_stats(z)
        out["out"], out["rstd"] = (z - mean) * rstd, rstd
    elif epi in ("PRELU_LN_BWD", "PRELU_LN_BWD_SEG"):
        xh, gam, al = c("aux"), c("epi_gamma"), c("epi_alpha")
        y = xh * gam + c("epi_beta")
        neg = t["aux"].double() * t["epi_gamma"].double() + t["epi_beta"].double() < 0       # (the branch is an input property)
        dy = torch.where(neg, al * acc, acc)
        out["out"] = ln_bwd(dy, xh, gam, c("aux_stats")[:, None])
        out["dgamma"], out["dbeta"] = (dy * xh).sum(0, keepdim=True), dy.sum(0, keepdim=True)
        out["dalpha"] = torch.where(neg, acc * y, torch.zeros_like(y)).sum().reshape(1, 1)
        out["_dalpha_terms"] = torch.where(neg, acc * y, torch.zeros_like(y)).abs().sum().reshape(1, 1)
        if epi == "PRELU_LN_BWD_SEG":
            out["agg"] = seg_sum(out["out"])
    elif epi == "RELU_MASK":
        out["out"] = acc * (t["aux"] > 0)
    elif epi == "ROWLN_BWD":
        st, gam = c("aux_stats"), c("epi_gamma")
        xh = (c("aux") - st[:, :1]) * st[:, 1:]
        out["out"] = ln_bwd(acc, xh, gam, st[:, 1:]) + (c("res") if "res" in t else 0)
        out["dgamma"], out["dbeta"] = (acc * xh).sum(0, keepdim=True), acc.sum(0, keepdim=True)
    elif epi == "PRELU_BWD":
        z = c("aux")
        out["out"] = torch.where(t["aux"] >= 0, acc, c("epi_alpha") * acc)
        out["dalpha"] = torch.where(t["aux"] < 0, acc * z, torch.zeros_like(z)).sum().reshape(1, 1)
        out["_dalpha_terms"] = torch.where(t["aux"] < 0, acc * z, torch.zeros_like(z)).abs().sum().reshape(1, 1)
    elif epi == "SEGSUM":
        msg = acc + c("bias") if "bias" in t else acc
        out["agg"] = seg_sum(msg)
        if "res" in t:
            out["out"] = msg + c("res")
    if not spec.get("partials"):                      # (no partial rows asked for: the parameter gradients are not produced)
        for k in ("dgamma", "dbeta", "dalpha", "_dalpha_terms"):
            out.pop(k, None)
    return out


def row_err(got, ref64, scale=None):
    """Worst row of max|got - ref| / max|ref| (each row by its OWN largest reference magnitude, or by `scale` [rows, 1]);
    inf where a row of zeros is not reproduced exactly or `got` holds a NaN."""
    got, ref64 = got.double().reshape(ref64.shape), ref64.double()
    d = (got - ref64).abs().amax(1)
    s = (ref64.abs().amax(1) if scale is None else scale.double().reshape(-1))
    r = torch.where(s > 0, d / s.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))
    r = torch.where(torch.isnan(d), torch.full_like(d, math.inf), r)
    return float(r.max())


def errors(spec, got, ref):
    """{output: worst row error} of a case; the row mean of stats_out is judged on the row's size (it cancels to ~0).
    dalpha, one scalar over M x N signed terms, is judged twice: against its own magnitude like everything else (the issue's
    measure; how far the sum cancels decides the figure, see BOUNDS) and, as "dalpha/terms", against the sum of the |terms| -
    the measure that does not depend on the cancellation, held to TOL.  (`_` keys of a reference are scales, not outputs.)"""
    e = {}
    for k, r in ref.items():
        if k.startswith("_"):
            continue
        scale = ref["out"].abs().amax(1) if k == "stats_mean" else None
        e[k] = row_err(got[k], r, scale)
    if "_dalpha_terms" in ref:
        e["dalpha/terms"] = row_err(got["dalpha"], ref["dalpha"], ref["_dalpha_terms"])
    return e


def outputs(ref):
    return {k for k in ref if not k.startswith("_")}


def fp32_baseline(spec, dev="cpu"):
    """The same formula in plain fp32 torch against float64 on the same operands: what BOUNDS is derived from."""
    t = make_inputs(spec, dev)
    return errors(spec, reference(spec, t, torch.float32), reference(spec, t, torch.float64))


# ---- the cases of a row ------------------------------------------------------------------------------------------------------
# Shapes: (which M, which N, K of the vector families, (K, left pad of A) of the generic ones - a pad of 5 misaligns A, K = 5 / 41
# are no multiples of 4), k1 = width of a first, GATHERED K-segment (its boundary falls inside the first k-chunk).
#   M "one": one row in the last row tile, "short": one row short of full; N "full": fills the column tiles, "ragged"
CASE_SHAPES = [
    dict(m="one", n="full", K=4, generic=(5, 4)),
    dict(m="short", n="ragged", K=100, generic=(41, 4)),                       # K % 32 != 0
    dict(m="one", n="ragged", K=160, generic=(64, 5)),                         # K % 32 == 0: the buffer-addressed staging
    dict(m="short", n="full", K=4, generic=(4, 5)),
    dict(m="one", n="ragged", K=64, generic=(41, 4), k1=(20, 5)),               # two K-segments (vector, generic first width)
]
CASE_KMAX = dict(m="short", n="full", K=GEMM_KMAX)                             # sixth case of the LayerNorm prologues
CASE_ADD = dict(m="one", n="ragged", K=100, add=True)                          # sixth case of the LayerNorm epilogue
# Optional operands of case 0..5 by epilogue (absent = off).  res_col0 = -64: the residual covers the last 64 columns.
# stats / norm apply where the row allows them: always when the row needs one of them for its column tile ("stats" rows; every
# case then has at least one), else only for N <= 128 - there `bare` marks the case that runs without either.
OPTIONAL = {
    "BIAS_ACT": [dict(bias=True, act=0, res=True, stats=True),
                 dict(act=1, norm=True),
                 dict(bias=True, act=2, res=True, stats=True),
                 dict(act=0, res=True, res_col0=-64, norm=True, bare=True),
                 dict(bias=True, act=1, res=True, res_pre=True, stats=True),
                 dict(act=2, res=True, stats=True, norm=True)],
    "LN": [dict(bias=True), dict(), dict(bias=True), dict(), dict(bias=True), dict()],
    "ROWLN_BWD": [dict(res=True, partials=True), dict(), dict(res=True, partials=True), dict(partials=True), dict(res=True),
                  dict(partials=True)],
    "PRELU_LN_BWD": [dict(partials=True), dict(), dict(partials=True), dict(), dict(partials=True), dict()],
    "PRELU_BWD": [dict(partials=True), dict(), dict(partials=True), dict(), dict(partials=True), dict()],
    "RELU_MASK": [dict()] * 6,
    "SEGSUM": [dict(bias=True, res=True), dict(mean=True), dict(bias=True, res=True), dict(res=True, mean=True), dict(bias=True),
               dict(res=True, mean=True)],
    "PRELU_LN_BWD_SEG": [dict(partials=True), dict(mean=True), dict(partials=True), dict(mean=True), dict(partials=True),
                         dict(mean=True)],
}


def cases(row):
    """The case specs of one ROWS entry: CASE_SHAPES, then K = GEMM_KMAX for a LayerNorm prologue or the gathered addends of
    the LayerNorm epilogue, each with the optional operands OPTIONAL gives its position."""
    family, pro, epi, extra, kernel, (nf, mf1, mf2), (nr, mr1, mr2) = row
    wl, vec = FAMILIES[family][:2]
    shapes = list(CASE_SHAPES)
    if vec and pro in ("LN_PRELU", "ROWLN"):
        shapes.append(CASE_KMAX)
    if epi == "LN":
        shapes.append(CASE_ADD)
    out = []
    for i, (c, opt) in enumerate(zip(shapes, OPTIONAL[epi])):
        N = nf if c["n"] == "full" else nr
        M = {("one", nf): mf1, ("short", nf): mf2, ("one", nr): mr1, ("short", nr): mr2}[(c["m"], N)]
        K, left = (c["K"], 4) if vec else c["generic"]
        s = dict(M=M, N=N, K=K, a_left=left, wl=wl, vec=vec, pro=pro, epi=epi, kernel=kernel, family=family)
        if "k1" in c:
            s["k1"] = c["k1"][0 if vec else 1]
        if c.get("add"):
            s["add"] = True
        s.update({k: v for k, v in opt.items() if k not in ("stats", "norm", "bare", "res_col0")})
        if "res_col0" in opt:
            s["res_col0"] = N + opt["res_col0"]
        if epi == "BIAS_ACT" and (extra or (N <= 128 and not opt.get("bare"))):
            s["stats"], s["norm"] = bool(opt.get("stats")), bool(opt.get("norm"))
        out.append(s)
    return out


def prepare(o, lib, spec, t):
    """The descriptor of one case with every operand a view into a larger buffer: inputs inside NaN, outputs inside the
    sentinel.  Returns (descriptor, {name: Guarded}, whether `out` is written, partial rows, what must stay alive)."""
    from dostransformer_amd import _abi
    M, N, K, epi = spec["M"], spec["N"], spec["K"], spec["epi"]
    dev = t["w"].device
    keep = []

    def pad(k, **kw):
        if k not in t:
            return None
        p = Padded(t[k], **kw)
        keep.append(p)
        return p.view

    def vec1(k):                                   # a [n] vector inside NaN: 4 floats in front (16-byte aligned), 4 behind
        if k not in t:
            return None
        p = Padded(t[k][None, :], top=0, bottom=0)
        keep.append(p)
        return p.view[0]

    if "a" in t:
        segs = [o.seg(pad("a", left=spec.get("a_left", 4)))]
    else:
        nx = t["x"].shape[0]
        xpad = pad("x")                            # 64 NaN rows behind the table; the index padding points at them
        idx = torch.full((1 + M + 64,), nx + 1, device=dev, dtype=torch.int32)
        idx[1:1 + M] = t["idx"]
        keep.append(idx)
        segs = [o.seg(xpad, rmap=o.rowmap(idx=idx[1:1 + M])), o.seg(pad("a1", left=spec.get("a_left", 4)))]
    kw = dict(w_layout=spec["wl"], pro=getattr(_abi, "DOSX_PRO_" + spec["pro"]), epi=getattr(_abi, "DOSX_EPI_" + epi))
    for k in ("pro_gamma", "pro_beta", "bias", "epi_gamma", "epi_beta"):
        if k in t:
            kw[k] = vec1(k)
    for k in ("pro_alpha", "epi_alpha"):
        if k in t:
            kw[k] = t[k]
    if "pro_stats" in t:
        kw["pro_stats"] = pad("pro_stats", left=0, right=0)
    if "aux" in t:
        kw["aux"] = pad("aux")
        kw["aux_stats"] = pad("aux_stats", left=0, right=0) if "aux_stats" in t else None
    if "res" in t:
        kw["res"] = pad("res")
        kw["res_col0"], kw["res_pre"] = spec.get("res_col0", 0), bool(spec.get("res_pre"))
    if epi == "BIAS_ACT":
        kw["act"], kw["act_slope"] = spec.get("act", 0), spec.get("slope", 0.01)
    if "add_pq" in t:
        pa, qa = Padded(t["add_pq"][:, :N].contiguous()), Padded(t["add_pq"][:, N:].contiguous())      # each table inside its own NaN
        keep += [pa, qa]
        ips = []
        for k in ("add_ip", "add_iq"):             # index rows behind M point at the NaN rows behind the table
            ix = torch.full((1 + M + 64,), t["add_pq"].shape[0] + 1, device=dev, dtype=torch.int32)
            ix[1:1 + M] = t[k]
            keep.append(ix)
            ips.append(ix[1:1 + M])
        kw.update(add_p=pa.view, add_q=qa.view, add_ip=ips[0], add_iq=ips[1])
    G = {}
    want_out = epi != "SEGSUM" or "res" in t
    G["out"] = Guarded(M, N, dev)
    if spec.get("stats"):
        G["stats"] = Guarded(M, 2, dev, left=0, right=0)
        kw["stats_out"] = G["stats"].view
    if spec.get("norm"):
        G["norm"], G["norm_rstd"] = Guarded(M, N, dev), Guarded(M, 1, dev, left=0, right=0)
        kw["norm_out"], kw["norm_rstd"] = G["norm"].view, G["norm_rstd"].view
    if epi == "LN":
        G["rstd"] = Guarded(M, 1, dev, left=0, right=0)
        kw["aux_out"] = G["rstd"].view
    prow = 0
    if spec.get("partials"):
        e = getattr(_abi, "DOSX_EPI_" + epi)
        prow = spec["graph"]["tiles"].shape[1] - 1 if "graph" in spec else lib.dosx_gemm_partial_rows(M, N, e)
        # guard columns between the column sums and dalpha (the last float of a row) - but for the node-aligned tiles, where a
        # slot without rows zeroes its whole partial row
        pld = {"PRELU_BWD": 4, "PRELU_LN_BWD_SEG": 2 * N + 1}.get(epi, 2 * N + 4)
        G["partials"] = Guarded(prow, pld, dev, left=0, right=0)
        ok = torch.zeros(pld, dtype=torch.bool, device=dev)
        if epi != "PRELU_BWD":
            ok[:2 * N] = True
        if epi != "ROWLN_BWD":
            ok[pld - 1] = True
        G["partials"].allow(ok)
        kw["partials"], kw["partial_ld"] = G["partials"].view, pld
    if "graph" in spec:
        gr = spec["graph"]
        G["agg"] = Guarded(gr["n"], N, dev, left=0, right=0)
        kw.update(seg_tile=gr["tiles"], seg_rowptr=gr["rowptr"], seg_scale=t.get("seg_scale"), seg_agg=G["agg"].view)
    g = o._gemm_desc(M, N, segs, pad("w"), G["out"].view if want_out else None, **kw)
    return g, G, want_out, prow, keep


def run(o, lib, spec, t):
    """Launch one case.  Returns (outputs by name, kernel named, {buffer: guards intact}, partial rows)."""
    g, G, want_out, prow, keep = prepare(o, lib, spec, t)
    named = kernel_name(lib, g)
    o._call("dosx_gemm", C.byref(g), o._stream())
    torch.cuda.synchronize()
    return collect(spec, G, spec["N"], want_out), named, {k: v.intact() for k, v in G.items()}, prow


def run_pair(o, lib, specs, ts):
    """dosx_gemm_pair on two prepared cases: ([outputs], [{buffer: guards intact}])."""
    ps = [prepare(o, lib, s, t) for s, t in zip(specs, ts)]
    # dosx_gemm_pair falls back to two dosx_gemm launches when the problems do not pair, and nothing a caller sees tells the two
    # apart - so what it pairs on is asserted on the REAL descriptors: vector staging on both, the same column tile, and the
    # kernels the specs name (the one-height pair: the plan of all rows together; the two-height pair: each problem's own)
    names = [kernel_name(lib, p[0]) for p in ps]
    assert all(n.split(", ")[4] == "1" for n in names) and len({n.split(", ")[1] for n in names}) == 1, names
    if specs[0]["epi"] == "BIAS_ACT":
        both = type(ps[0][0]).from_buffer_copy(ps[0][0])
        both.M = ps[0][0].M + ps[1][0].M
        assert kernel_name(lib, both) == specs[0]["kernel"] == specs[1]["kernel"], (kernel_name(lib, both), specs[0]["kernel"])
    else:
        assert names == [s["kernel"] for s in specs], names
    o._call("dosx_gemm_pair", C.byref(ps[0][0]), C.byref(ps[1][0]), o._stream())
    torch.cuda.synchronize()
    return ([collect(s, p[1], s["N"], p[2]) for s, p in zip(specs, ps)], [{k: v.intact() for k, v in p[1].items()} for p in ps])


def collect(spec, G, N, want_out=True):
    """The outputs of a finished case by reference() name; partial rows summed over the workgroups in float64."""
    got = {}
    if want_out:
        got["out"] = G["out"].view
    if "stats" in G:
        got["stats_mean"], got["stats_rstd"] = G["stats"].view[:, :1], G["stats"].view[:, 1:]
    if "norm" in G:
        got["norm"], got["norm_rstd"] = G["norm"].view, G["norm_rstd"].view
    if "rstd" in G:
        got["rstd"] = G["rstd"].view
    if "agg" in G:
        got["agg"] = G["agg"].view
    if "partials" in G:
        p = G["partials"].view.double().sum(0, keepdim=True)
        if spec["epi"] != "PRELU_BWD":
            got["dgamma"], got["dbeta"] = p[:, :N], p[:, N:2 * N]
        if spec["epi"] != "ROWLN_BWD":
            got["dalpha"] = p[:, -1:]
    return got
