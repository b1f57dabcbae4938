"""csrc/launch_state.h -- the per-device cell every launch site keeps its LDS grant and resident-workgroup count in, and
the grid rule of the persistent kernels -- compiled for the host into a stand-alone program
(tests/native/launch_state_harness.cpp) against stubbed device queries: once with AddressSanitizer and
UndefinedBehaviorSanitizer, once with ThreadSanitizer (eight threads fill and read the cells of two devices).  The same
header is what the HIP launchers include."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module", params=["address,undefined", "thread"])
def harness(request, tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is needed to build tests/native/launch_state_harness.cpp"
    exe = tmp_path_factory.mktemp("launch_state") / "harness"
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread",
                           f"-fsanitize={request.param}", "-fno-sanitize-recover=all",
                           "-I", str(ROOT / "pyannote-audio_amd" / "csrc"),
                           str(ROOT / "tests" / "native" / "launch_state_harness.cpp"), "-o", str(exe)])
    return request.param, exe


def test_cells_rules_and_grid(harness):
    sanitizer, exe = harness
    rc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    if sanitizer == "thread" and rc.returncode != 0 and "FATAL: ThreadSanitizer" in rc.stderr \
            and "launch state held" not in rc.stdout and "WARNING: ThreadSanitizer" not in rc.stderr:
        # the runtime itself did not start (e.g. an address-space layout it does not support): nothing was checked
        pytest.skip("ThreadSanitizer runtime refused to start: " + rc.stderr.strip().splitlines()[0])
    assert rc.returncode == 0, rc.stdout + rc.stderr
    assert "launch state held" in rc.stdout
