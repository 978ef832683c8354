"""csrc/blockops.hpp — the bookkeeping primitives of the ragged calls, one definition each — as far as the text of csrc can show it: the
header is part of the build's staleness check, every primitive is defined once under csrc, every .hip file that calls one includes the
header, and the header holds nothing of the permutation.  (What the primitives compute is held by the suites of their callers: the scans
by test_scan_width_*, the claim table by test_forest_update_* and test_forest_journal_*, the sorts by test_ragged_* and
test_forest_openings_*, all of them by test_forest_walk_*.)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")

# defined in blockops.hpp ...
DEVICE = ("block_exclusive", "scan_tile_row", "last_at_or_below", "claim", "append_place", "bucket_hist", "bucket_scatter")
CONSTANTS = ("CLAIM_EMPTY", "CLAIM_MIN_SLOTS")
# ... and the two that belong elsewhere: the host's shift of a table size, and the list record next to the closed forms
ELSEWHERE = {"shift_of": "forest_update.h", "record": "forest_node.hpp"}
USERS = {"ragged.hip", "forest_ragged.hip", "forest_openings.hip", "forest_update.hip", "forest_journal.hip", "forest_append.hip",
         "multiproof.hip", "forest_multiproof.hip"}
SCAN_LOOP = "for (unsigned off = 1; off <"


def _code(name):
    """the file without its // comments"""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def _sources():
    return sorted(n for n in os.listdir(CSRC) if n.endswith((".h", ".hpp", ".hip", ".cpp")))


def _definitions(fn):
    """{file: count} of the lines under csrc that define function `fn`: a function specifier, then the name and its parameter list"""
    pat = re.compile(r"^\s*(?:__device__|__host__|static|inline)\b[^\n;(]*\b%s\s*\(" % fn, re.M)
    found = {n: len(pat.findall(_code(n))) for n in _sources()}
    return {n: c for n, c in found.items() if c}


def test_header_is_in_the_staleness_check():
    from poseidon252_amd import build as b
    assert "blockops.hpp" in b.HEADERS and os.path.exists(os.path.join(CSRC, "blockops.hpp"))
    assert "blockops.hpp" not in b.SOURCES


def test_each_primitive_is_defined_once():
    for fn in DEVICE:
        assert _definitions(fn) == {"blockops.hpp": 1}, (fn, _definitions(fn))
    for fn, home in ELSEWHERE.items():
        assert _definitions(fn) == {home: 1}, (fn, _definitions(fn))
    for name in CONSTANTS:
        found = {n: len(re.findall(r"\bconstexpr\b[^\n;]*\b%s\s*=" % name, _code(n))) for n in _sources()}
        assert {n: c for n, c in found.items() if c} == {"blockops.hpp": 1}, (name, found)
    # the copies' own names are gone
    for n in _sources():
        assert not re.search(r"\bF[UJ]_(EMPTY|MIN_SLOTS)\b", _code(n)), n


def test_every_caller_includes_the_header():
    call = re.compile(r"\b(?:%s)\s*[(<]" % "|".join(DEVICE + CONSTANTS))
    users = set()
    for n in _sources():
        if n == "blockops.hpp":
            continue
        src = open(os.path.join(CSRC, n)).read()
        if call.search(_code(n)) or any(re.search(r"\b%s\b" % c, _code(n)) for c in CONSTANTS):
            assert '#include "blockops.hpp"' in src, n
            users.add(n)
        else:
            assert '#include "blockops.hpp"' not in src, n
    assert users == USERS, sorted(users ^ USERS)


def test_the_block_scan_loop_is_written_where_it_has_to_be():
    # once in the header, once in k_ragged_scan (an inclusive scan of per-thread sums), twice in forest_multiproof.hip (the two segmented
    # forms: block_seg_scan and the three-array scan of k_fm_scan_tiles)
    found = {n: _code(n).count(SCAN_LOOP) for n in _sources()}
    assert {n: c for n, c in found.items() if c} == {"blockops.hpp": 1, "ragged.hip": 1, "forest_multiproof.hip": 2}, found
    fm = _code("forest_multiproof.hip")
    assert "block_seg_scan" in fm and "seg_combine" in fm


def test_header_is_device_only_and_holds_nothing_of_the_permutation():
    src = open(os.path.join(CSRC, "blockops.hpp")).read()
    code = _code("blockops.hpp")
    for word in ("hades_permute", "node_digest", "asm"):
        assert word not in src, word
    assert re.findall(r'#include\s+"([^"]+)"', code) == []  # none of the project's headers: the field and the permutation stay out
    bodies = re.findall(r"^[^\n;]*\)\s*\{\s*$", code, re.M)
    functions = [ln for ln in bodies if re.match(r"\s*(?:__device__|__host__|static|inline|template)\b", ln) or "__forceinline__" in ln]
    assert len(functions) == len(DEVICE), functions
    assert all("__device__" in ln and "__host__" not in ln and "__global__" not in ln for ln in functions), functions
    assert "__global__" not in code and "hipLaunchKernelGGL" not in code  # the kernels stay in their own files
