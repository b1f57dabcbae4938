"""tools/build_variants.py: a variant that builds the work tree's source (revision None) must name only -D switches
that this source still has.  A flag the source does not know changes nothing, and the "variant" would be the product
kernel under another name.  Variants of switches that left the sources carry the last revision that had them."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_table():
    spec = importlib.util.spec_from_file_location("build_variants", os.path.join(ROOT, "tools", "build_variants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.VARIANTS


def test_work_tree_variants_name_switches_their_source_has():
    csrc = os.path.join(ROOT, "pyannote-audio_amd", "csrc")
    for tag, (src, flags, rev) in load_table().items():
        assert os.path.exists(os.path.join(csrc, src)), f"{tag}: no source {src}"
        if rev is not None:
            continue
        with open(os.path.join(csrc, src)) as fp:
            text = fp.read()
        for flag in flags.split():
            if flag.startswith("-D"):
                name = flag[2:].split("=", 1)[0]
                assert re.search(rf"\b{re.escape(name)}\b", text), (
                    f"variant {tag}: {src} of the work tree does not know {name}; pin the variant to the last "
                    f"revision that does")
