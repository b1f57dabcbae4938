"""csrc/workspace.h -- pa::Carver, the one description of every caller-allocated workspace -- compiled for the host
with AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program (tests/native/carver_harness.cpp):
the sizing pass and the carving pass agree on bytes(), every block is aligned as asked, the blocks are disjoint, in
order and inside the buffer, and writing all of them in a buffer of exactly bytes() bytes is clean.  The same header
is what the HIP entry points include."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("carver") / "harness"
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", str(ROOT / "pyannote-audio_amd" / "csrc"),
                           str(ROOT / "tests" / "native" / "carver_harness.cpp"), "-o", str(exe)])
    return exe


def test_sizing_and_carving_agree_and_every_block_is_whole(harness):
    rc = subprocess.run([str(harness)], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stdout + rc.stderr
    assert "sequences held" in rc.stdout
