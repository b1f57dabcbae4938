"""The table of tests/stream_contract.py against include/pyannote_amd.h: no entry point with a `void* stream` parameter is
unclassified, no row names a function the header lacks, and a `waits` row is one the header itself declares an exception
to "nothing synchronises" -- in the function's own comment and in the Conventions paragraph.  No GPU, no library."""
import re

import stream_contract as sc


def _header():
    return sc.HEADER.read_text()


def test_parser_sees_every_declaration():
    """the parser against a plain scan of the text: every `pa_name(` that is followed by a `;` before any `{`"""
    text = _header()
    decls = sc.parse_header(text)
    names = [d.name for d in decls]
    assert len(names) == len(set(names))
    body = re.sub(r"/\*.*?\*/", " ", text[text.index('extern "C" {'):], flags=re.S)
    plain = set(re.findall(r"\b(pa_\w+)\s*\(", body))
    assert set(names) == plain
    assert {"pa_version", "pa_seg_forward", "pa_gallery_pairs_f64", "pa_winograd_pack_host"} <= set(names)
    taking = sc.stream_taking(decls)
    assert "pa_seg_forward" in taking and "pa_version" not in taking and "pa_winograd_pack_host" not in taking
    # a parameter list is kept whole: the stream is the last parameter of every function that takes one
    for d in decls:
        if d.name in taking:
            assert re.search(r"void\s*\*\s*stream$", d.params), d


def test_every_stream_taking_entry_point_has_a_row():
    decls = sc.parse_header(_header())
    declared = set(sc.stream_taking(decls))
    rows = {r.name for r in sc.ROWS}
    assert declared - rows == set(), "entry points with a stream parameter and no row in tests/stream_contract.py"
    assert rows - declared == set(), "rows for functions the header does not declare with a stream parameter"
    assert len(declared) >= 90


def test_rows_are_well_formed():
    ids = [sc.row_id(r) for r in sc.ROWS]
    assert len(ids) == len(set(ids)), "two rows with the same name and variant"
    for r in sc.ROWS:
        assert r.cls in (sc.ASYNC, sc.WAITS) and callable(r.build), r
    # a function has several rows only under distinct variants, and only pa_kmeans_f64 is in both classes
    both = {r.name for r in sc.ROWS if r.cls == sc.WAITS} & {r.name for r in sc.ROWS if r.cls == sc.ASYNC}
    assert both == {"pa_kmeans_f64"}


def test_waits_rows_are_the_exceptions_the_header_declares():
    text = _header()
    decls = sc.parse_header(text)
    waits = {r.name for r in sc.ROWS if r.cls == sc.WAITS}
    assert waits == {"pa_binarize_regions", "pa_regions_sweep_count", "pa_regions_sweep_emit",
                     "pa_binarize_regions_files_count", "pa_binarize_regions_files_emit", "pa_kmeans_f64"}
    for name in waits:
        comment = sc._squash(sc.covering_comment(decls, name))
        assert any(words in comment for words in sc.WAITS_WORDS), f"{name}: its header comment does not say that it waits"
    # ... and the other way round: a comment that says so belongs to a `waits` row (pa_prof_report takes no stream)
    for d in decls:
        if d.name in sc.stream_taking(decls) and d.comment and d.name not in waits:
            own = sc._squash(d.comment)
            covered = {n for n in waits if sc.covering_comment(decls, n) == d.comment}
            assert covered or not any(words in own for words in ("waits for the stream", "wait for the stream")), d.name
    paragraph = sc._squash(sc.conventions(text))
    assert "nothing synchronises" in paragraph and "no hidden allocation" in paragraph
    for name in waits:
        assert name in paragraph, f"{name} is not named among the exceptions of the Conventions paragraph"
    # no other entry point is named there as an exception
    named = set(re.findall(r"\bpa_\w+", paragraph)) - {"pa_last_error"}
    assert named & set(sc.stream_taking(decls)) == waits


def test_a_new_or_reclassified_declaration_is_noticed():
    """the three edits the table must not survive, made on a copy of the header's text"""
    text = _header()
    rows = {r.name for r in sc.ROWS}
    added = text.replace("int pa_version(void);", "int pa_version(void);\nint pa_new_kernel(const float* x, void* stream);")
    assert set(sc.stream_taking(sc.parse_header(added))) - rows == {"pa_new_kernel"}
    removed = re.sub(r"int pa_w2v_axpy\([^;]*;", "", text)
    assert rows - set(sc.stream_taking(sc.parse_header(removed))) == {"pa_w2v_axpy"}
    silent = text.replace("The call waits for the\n * stream (it reads the counts back to check the capacity).", "")
    assert silent != text
    comment = sc._squash(sc.covering_comment(sc.parse_header(silent), "pa_binarize_regions"))
    assert not any(words in comment for words in sc.WAITS_WORDS)
