"""csrc/emb_conv_s2_geom.h -- the integer geometry of the stride-2 convolution kernel k_conv3x3_s2 (LDS images and
their bank swizzle, per-lane LDS-DMA source offsets, fragment read addresses, piece counts) -- compiled UNCHANGED for
the host and replayed for every piece, wave, lane and tap of both instantiations
(tests/native/conv_s2_geom_harness.cpp): every patch element and weight of a stage is written by exactly one DMA
lane, every fragment read returns the element its (tap, pixel, channel) names or a hardware zero outside the image,
halo and padding lanes carry the out-of-bounds offset, every ds_read_b128 is conflict-free under the hardware's
lane-group rule, and the piece counts are the constants the kernel's waits and issue slots are built from."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_dma_layout_matches_fragment_reads_and_is_conflict_free(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "geom_s2"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wno-unknown-pragmas",
                           "-I", str(ROOT / "pyannote-audio_amd" / "csrc"),
                           str(ROOT / "tests" / "native" / "conv_s2_geom_harness.cpp"), "-o", str(exe)])
    rc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert rc.returncode == 0, rc.stdout + rc.stderr
