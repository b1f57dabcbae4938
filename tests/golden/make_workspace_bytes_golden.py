"""Regenerates tests/golden/workspace_bytes_v1.json: the table of tests/test_workspace_layouts_cpu.py -- (function,
arguments, environment) -> bytes -- as the size functions of a GIVEN build of the library return it.  The recorded file
comes from the commit BEFORE the workspace layouts moved onto pa::Carver (csrc/workspace.h), never from the code the
test checks:

    git worktree add ../before <that commit> && (cd ../before && python __graft_entry__.py)
    PA_LIB=../before/pyannote-audio_amd/libpyannote_amd.so python tests/golden/make_workspace_bytes_golden.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PATH = os.path.join(ROOT, "tests", "golden", "workspace_bytes_v1.json")

if __name__ == "__main__":
    if not os.environ.get("PA_LIB"):
        raise SystemExit("PA_LIB must name the library of the commit the values are recorded from")
    if not os.path.exists(PATH):
        open(PATH, "w").write("[]")          # (the test module reads the file on import)
    import pyannote_audio_amd.ffi as ffi
    from test_workspace_layouts_cpu import table
    rows = table(ffi.load(), ffi)
    with open(PATH, "w") as fp:
        fp.write("[\n" + ",\n".join(json.dumps(row, separators=(",", ":")) for row in rows) + "\n]\n")
    print(f"wrote {PATH}: {len(rows)} values from {ffi.lib_path()}")
