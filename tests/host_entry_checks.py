"""Shared by the CPU-side tests of the sample statistics (nearest neighbours, kernel MMD, DTW, Sinkhorn, Frechet / PCA):
the host regions and refusal sweeps of their ``test_argument_errors_before_device_work`` tests, and the source check that
the host prologue of their entry points is stated once.  No GPU: every refusal comes before any device work, and the one
accepted call of ``checks_work`` is made only where there is no device to launch on."""
import os
import re

import numpy as np
import torch

INVALID, UNSUPPORTED, HIP = -1, -2, -4


class HostBuffers:
    """Distinct 16-byte aligned host regions standing where device buffers would: every refusal comes before any device
    work, so none of them is ever read by a kernel.  ``untouched`` checks that nothing changed."""

    def __init__(self, **sizes):
        self.store = {}
        for name, size in sizes.items():
            raw = np.full(size + 16, 0xA5, np.uint8)
            self.store[name] = (raw, (-raw.ctypes.data) % 16)

    def __getattr__(self, name):
        raw, off = self.store[name]
        return raw.ctypes.data + off

    def untouched(self):
        return all((raw == 0xA5).all() for raw, _ in self.store.values())


def refuses_every_alias(call, written, read):
    """``written`` and ``read`` map the keyword of each region the entry takes to the address ``call`` passes by default
    (None: an optional region left out).  Every written region is moved onto the start of every other region, written or
    read, the workspace among the written ones: each of these calls is refused."""
    regions = {**written, **read}
    assert len(regions) == len(written) + len(read)
    count = 0
    for w in written:
        for other, addr in regions.items():
            if other != w and written[w] is not None and addr is not None:
                assert call(**{w: addr}) == INVALID, (w, other)
                count += 1
    return count


def checks_work(call, work, need, work_kw="work", nbytes_kw="nbytes"):
    """A misaligned workspace and one a byte short are refused; exactly ``need`` bytes pass every check, which without a
    device shows as the HIP error of the first launch (with one, the GPU tests make this call: the Python layer passes
    exactly the need)."""
    assert need > 0 and need % 16 == 0
    for shift in (4, 8):
        assert call(**{work_kw: work + shift}) == INVALID, shift
    assert call(**{nbytes_kw: need - 1}) == INVALID
    if not torch.cuda.is_available():
        assert call(**{nbytes_kw: need}) == HIP


SOURCES = ("ffd_neighbours.hip", "ffd_mmd.hip", "ffd_dtw.hip", "ffd_sinkhorn.hip", "ffd_pca.hip")


def one_host_prologue(csrc):
    """The host pieces have one statement each: the workspace helpers in ffd_workspace.h, the pair-set prologue in
    ffd_pairtile.h's host section (which includes the former), and none of the five sources defines a shape-limit pair, a
    spill helper, an overlap test or a column-mean launch of its own, or spells the workspace test out."""
    helper = open(os.path.join(csrc, "ffd_workspace.h")).read()
    shared = open(os.path.join(csrc, "ffd_pairtile.h")).read()
    make = open(os.path.join(csrc, "Makefile")).read()
    assert '#include "ffd_workspace.h"' in shared and "hip" not in helper.split("#pragma once")[1].lower()
    assert re.search(r"^ffd_neighbours\.o .*\.isa/ffd_pca\.s: ffd_pairtile\.h ffd_workspace\.h$", make, re.M)
    for piece in ("size_t nn_up(", "struct Carver {", "bool work_ok(", "bool regions_meet(", "bool regions_clash("):
        assert helper.count(piece) == 1 and piece not in shared, piece
    for piece in ("bool nn_shape_ok(", "bool nn_shape_supported(", "size_t nn_spill_bytes(", "size_t nn_colpart_bytes(",
                  "void nn_launch_colmean(", "PairPlan nn_pair_plan(", "PairRows nn_centre_pair("):
        assert shared.count(piece) == 1 and piece not in helper, piece
    for launch in ("hipLaunchKernelGGL(k_nn_colpart", "hipLaunchKernelGGL(k_nn_colmean<T>"):
        assert shared.count(launch) == 1, launch
    for source in SOURCES:
        text = open(os.path.join(csrc, source)).read()
        assert '#include "ffd_pairtile.h"' in text, source
        for pattern in (r"bool \w+\(int \w+, int \w+, int D\)",     # a shape-limit pair over (rows, rows, D)
                        r"\w+_spill_bytes\([^)]*\) \{",                # a spill helper's definition
                        r"hipFuncAttributeMaxDynamicSharedMemorySize",
                        r"_overlap\(",                                  # a pairwise overlap test or a loop over one
                        r"uintptr_t\)\s*work\b",                        # the workspace test spelled out
                        r"size_t o = 0;",                               # a plan carved by hand
                        r"hipLaunchKernelGGL\(k_nn_col(part|mean)"):
            assert not re.search(pattern, text), (pattern, source)
