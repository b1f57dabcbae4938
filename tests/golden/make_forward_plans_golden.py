"""Regenerates tests/golden/forward_plans_v1.json: the table of tests/test_forward_plans_cpu.py as the size and frame
functions of a GIVEN build of the library return it.  The recorded file comes from the commit BEFORE the forward entry
points shared their plans (csrc/forward_common.h), never from the code the test checks:

    git worktree add ../before <that commit> && (cd ../before && python __graft_entry__.py)
    PA_LIB=../before/pyannote-audio_amd/libpyannote_amd.so python tests/golden/make_forward_plans_golden.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PATH = os.path.join(ROOT, "tests", "golden", "forward_plans_v1.json")

if __name__ == "__main__":
    if not os.environ.get("PA_LIB"):
        raise SystemExit("PA_LIB must name the library of the commit the values are recorded from")
    if not os.path.exists(PATH):
        open(PATH, "w").write("{}")          # (the test module reads the file on import)
    import pyannote_audio_amd.ffi as ffi
    from test_forward_plans_cpu import table
    plans = table(ffi.load(), ffi)
    with open(PATH, "w") as fp:
        json.dump(plans, fp, separators=(",", ":"))
        fp.write("\n")
    print(f"wrote {PATH}: {sum(len(v) for v in plans.values())} values from {ffi.lib_path()}")
