"""Where the scaffolding of the per-call test files lives, as far as the text of tests/ can show it: no module of tests/ is another
one's library unless it is a helper (no import of a test module, scripts held in strings included); the compiler lines for tests/cpp
and the parser of a refusal table are helpers/percall.py's alone; the harness of the refusal programs is tests/cpp/refusal_table.hpp's
alone; no module of tests/ imports a bench tool and no bench tool another, and the geometry of a tree (testsupport/treeshape.py) and
the tools' clock probe (bench_tools/_common.py) are each defined once.  ("Adding a call: the test scaffolding", says which
helper a new call's test files use and where its model and its bench tool go.)"""
import os
import re

TESTS = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(TESTS, "cpp")
PERCALL = os.path.join("helpers", "percall.py")
# its own compiler line, with the sanitizers' flags, for its own program: not a mirror and not a refusal table
OWN_COMPILER_LINE = {"test_sanitizers.py"}


def _python_sources():
    out = {}
    for d, _, names in os.walk(TESTS):
        for n in names:
            if n.endswith(".py"):
                path = os.path.join(d, n)
                out[os.path.relpath(path, TESTS)] = open(path).read()
    return out


def test_no_module_imports_a_test_module():
    """`from test_x import ...` and `import test_x`, at the start of any line: those of child scripts kept in strings too"""
    pat = re.compile(r"^[ \t]*(?:from[ \t]+test_\w+[ \t]+import\b|import[ \t]+test_\w+)", re.M)
    sources = _python_sources()
    assert len(sources) > 80 and PERCALL in sources
    assert {n: pat.findall(s) for n, s in sources.items() if pat.search(s)} == {}


def test_compiler_lines_and_the_row_parser_are_the_helper_modules():
    names_cpp = re.compile(r'tests/cpp|"tests",\s*"cpp"')  # the directory, as a path or as the parts of a join
    rows = re.compile(r"^[ \t]*def _rows\b", re.M)
    sources = _python_sources()
    assert "def refusal_rows(" in sources[PERCALL] and '"g++"' in sources[PERCALL]
    for name, src in sources.items():
        if name not in (PERCALL, os.path.basename(__file__)) and name not in OWN_COMPILER_LINE:
            assert not ('"g++"' in src and names_cpp.search(src)), name  # a file that runs g++ and names the directory
        assert not rows.search(src), name


def test_refusal_harness_is_in_the_header_only():
    row_format, kinds = r'"%s\t%s\t%d\t%s\n"', "enum Kind"
    holders = {what: sorted(n for n in os.listdir(CPP) if what in open(os.path.join(CPP, n)).read()) for what in (row_format, kinds)}
    assert holders == {row_format: ["refusal_table.hpp"], kinds: ["refusal_table.hpp"]}
    programs = sorted(n for n in os.listdir(CPP) if n.endswith("_refusals.cpp"))
    assert len(programs) == 6
    for n in programs:
        assert '#include "refusal_table.hpp"' in open(os.path.join(CPP, n)).read(), n


# ---- the numpy models live in testsupport/, the tools measure, and the geometry of a tree is testsupport/treeshape.py's alone ----
BENCH_TOOLS = os.path.join(os.path.dirname(TESTS), "bench_tools")
SUPPORT = os.path.join(os.path.dirname(TESTS), "testsupport")
BENCH_IMPORT = re.compile(r"^[ \t]*(?:from[ \t]+\w+_bench[ \t]+import\b|import[ \t]+\w+_bench\b)", re.M)


def _tool_sources():
    return {os.path.join("bench_tools", n): open(os.path.join(BENCH_TOOLS, n)).read() for n in sorted(os.listdir(BENCH_TOOLS)) if n.endswith(".py")}


def _support_sources():
    return {os.path.join("testsupport", n): open(os.path.join(SUPPORT, n)).read() for n in sorted(os.listdir(SUPPORT)) if n.endswith(".py")}


def test_no_test_module_imports_a_bench_tool():
    """`from x_bench import ...`, `import x_bench` and a sys.path.insert that names bench_tools, at the start of any line: those of child
    scripts kept in strings too.  A test reaches a tool by running it as a child process."""
    path = re.compile(r"^[ \t]*sys\.path\.insert\(.*bench_tools", re.M)
    sources = dict(_python_sources(), **_support_sources())
    found = {n: BENCH_IMPORT.findall(s) + path.findall(s) for n, s in sources.items()}
    assert {n: f for n, f in found.items() if f} == {}


def test_no_bench_tool_imports_a_bench_tool():
    tools = _tool_sources()
    assert len(tools) > 20 and os.path.join("bench_tools", "_common.py") in tools
    assert {n: BENCH_IMPORT.findall(s) for n, s in tools.items() if BENCH_IMPORT.search(s)} == {}


def test_the_geometry_and_the_clock_probe_are_defined_once():
    """over tests/**/*.py, bench_tools/*.py and testsupport/*.py together: one depth, one levels_len (edgecases._levels_len asks the library on purpose and is no
    second definition of the arithmetic), one levels bound, one offsets-from-sizes, one clock_mhz"""
    sources = dict(_tool_sources(), **_support_sources(), **{os.path.join("tests", n): s for n, s in _python_sources().items()})
    for what, pat, home in (("depth", r"def _?depth\(", "testsupport/treeshape.py"), ("levels_len", r"def levels_len\(", "testsupport/treeshape.py"),
                            ("levels bound", r"def _?levels_bound\(", "testsupport/treeshape.py"), ("offsets", r"def _?(?:offsets|offs)\(", "testsupport/treeshape.py"),
                            ("clock_mhz", r"def _?clock_mhz\(", "bench_tools/_common.py")):
        holders = sorted(n for n, s in sources.items() if re.search(r"^[ \t]*" + pat, s, re.M))
        assert holders == [os.path.normpath(home)], (what, holders)
    own_levels_len = sorted(n for n, s in sources.items() if re.search(r"^[ \t]*def _levels_len\(", s, re.M))
    assert own_levels_len == [os.path.join("tests", "edgecases.py")] and "from poseidon252_amd import levels_len" in sources[own_levels_len[0]]


def test_treeshape_and_the_models_ask_neither_the_library_nor_tests_nor_tools():
    support = _support_sources()
    assert "poseidon252_amd" not in support[os.path.join("testsupport", "treeshape.py")]
    for name in ("treeshape.py", "forestappend.py", "forestupdate.py", "multiproofmodel.py", "soundness.py"):
        imports = re.findall(r"^[ \t]*(?:from|import)[ \t]+([\w.]+)", support[os.path.join("testsupport", name)], re.M)
        assert set(imports) <= {"numpy", ".", ".treeshape"}, (name, imports)
