"""Where the scaffolding of the per-call test files lives, as far as the text of tests/ can show it: no module of tests/ is another
one's library unless it is a helper (no import of a test module, scripts held in strings included); the compiler lines for tests/cpp
and the parser of a refusal table are helpers/percall.py's alone; the harness of the refusal programs is tests/cpp/refusal_table.hpp's
alone.  ("Adding a call: the test scaffolding", says which helper a new call's test files use.)"""
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
    assert len(programs) == 5
    for n in programs:
        assert '#include "refusal_table.hpp"' in open(os.path.join(CPP, n)).read(), n
