"""The scaffolding that every call's `test_<call>_cpu.py` / `test_<call>_gpu.py` pair shares, as plain functions: the refusal
program's table and its golden file, the ABI checks of a call's symbols, the C++ mirror program, the bench tool's --help."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CPP = os.path.join(ROOT, "tests", "cpp")
LIB_DIR = os.path.join(ROOT, "poseidon252_amd")
ERR_HIP = -4


def _gxx(source, exe, flags, include, lib_dirs, libs):
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + list(flags) + ["-I", include, os.path.join(CPP, source)] +
                          [x for d in lib_dirs for x in ("-L", d)] + ["-l" + l for l in libs] + ["-Wl,-rpath," + d for d in lib_dirs] + ["-o", exe])
    return exe


def refusal_rows(text):
    """(symbol, case, return code, message) of every line; what follows the library's own part of a P252_ERR_HIP message, from the
    first ": " on, is the HIP runtime's text and differs between machines"""
    rows = [line.split("\t") for line in text.splitlines()]
    assert all(len(r) == 4 for r in rows), [r for r in rows if len(r) != 4][:3]
    return [(r[0], r[1], int(r[2]), r[3].split(": ")[0] if int(r[2]) == ERR_HIP else r[3]) for r in rows]


def refusal_table(name, tmp_dir):
    """tests/cpp/<name>.cpp, compiled against the HIP headers and the library and run (it never reaches a device) -> its rows"""
    from poseidon252_amd import build as B
    exe = _gxx(name + ".cpp", os.path.join(str(tmp_dir), name), ("-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__"), os.path.join(B.ROCM, "include"),
               [LIB_DIR], ["poseidon252_hip"])
    return refusal_rows(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


def assert_rows_equal_golden(table, name):
    golden = refusal_rows(open(os.path.join(ROOT, "tests", "golden", name + ".txt")).read())
    assert [r[:2] for r in table] == [r[:2] for r in golden]  # the same cases in the same order
    assert [r for r, g in zip(table, golden) if r != g] == []


def check_abi_symbols(n_args):
    """{symbol: argument count}: each is declared in the header with that many arguments (a `size_t` return for the `_bound`s, `int`
    for the rest), exported, in _lib.ABI_SYMBOLS and _lib.PROTOTYPES, and in the Rust FFI, under ABI 9; sys.rs is the generator's"""
    from poseidon252_amd import _lib
    raw = open(os.path.join(ROOT, "include", "poseidon252_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define P252_ABI_VERSION 9\b", raw)
    L = ctypes.CDLL(_lib.LIB_PATH)
    sysrs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (p252_\w+)\((.*?)\)", sysrs)}
    for name, n in n_args.items():
        m = re.search(r"\b(int|size_t) %s\s*\((.*?)\);" % name, header, flags=re.S)
        assert m, name
        assert (m.group(1) == "size_t") == name.endswith("_bound"), name
        assert m.group(2).count(",") + 1 == n, name
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
        assert len(_lib.PROTOTYPES[name][0]) == n, name
        assert rust[name].count(":") == n, (name, rust[name])
    assert _lib.lib().p252_abi_version() == 9 and _lib.ABI_VERSION == 9
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return raw, header


def build_cpp_mirror(name, tmp_path, oracle=True, flags=("-Wall", "-Werror"), hip_runtime=False):
    """tests/cpp/<name>.cpp against the public header and the library (and the oracle's, and the HIP runtime's) -> the program"""
    dirs = [LIB_DIR] + ([os.path.join(ROOT, "oracle")] if oracle else []) + (["/opt/rocm/lib"] if hip_runtime else [])
    libs = ["poseidon252_hip"] + (["p252_oracle"] if oracle else []) + (["amdhip64"] if hip_runtime else [])
    exe = _gxx(name + ".cpp", os.path.join(str(tmp_path), name), flags, os.path.join(ROOT, "include"), dirs, libs)
    assert os.path.exists(exe)
    return exe


def run_cpp_mirror(exe, timeout=600):
    out = subprocess.run([exe], capture_output=True, timeout=timeout)
    assert out.returncode == 0, out.stdout.decode() + out.stderr.decode()
    return out.stdout.decode()


def bench_tool_parses(name, options=("--quick",)):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_tools", name + ".py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(o in r.stdout for o in options), r.stderr
