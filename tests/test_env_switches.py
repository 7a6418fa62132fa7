"""The environment switches are read in one place per language -- alfi_amd/csrc/env.h for libalfi_hip.so, alfi_amd/env.py for
the package -- and documented in one table; profiling events are recorded through the ProfScope
guard only.  Source-level checks and the accessors of the package; no GPU, no native library."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alfi_amd", "csrc")
PKG = os.path.join(ROOT, "alfi_amd")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _csrc_files():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp")))


def _pkg_files():
    return sorted(f for f in os.listdir(PKG) if f.endswith(".py"))


def test_getenv_only_in_env_header():
    offenders = [f for f in _csrc_files() if f != "env.h" and "getenv" in _read(os.path.join(CSRC, f))]
    assert offenders == []
    assert "getenv" in _read(os.path.join(CSRC, "env.h"))


def test_environ_read_of_alfi_names_only_in_env_module():
    """No other module of the package touches os.environ / os.getenv at all, except shared.py for TMPDIR (not a project switch)."""
    offenders = []
    for f in _pkg_files():
        if f == "env.py":
            continue
        for line in _read(os.path.join(PKG, f)).splitlines():
            code = line.split("#", 1)[0]
            if re.search(r"\benviron\b|\bgetenv\b|\bputenv\b", code) and not (f == "shared.py" and "TMPDIR" in code and "ALFI_" not in code):
                offenders.append((f, line.strip()))
    assert offenders == []


def _names_in_header():
    return set(re.findall(r'getenv\("(ALFI_[A-Z0-9_]+)"\)', _read(os.path.join(CSRC, "env.h"))))


def _names_in_module():
    return set(re.findall(r'"(ALFI_[A-Z0-9_]+)"', "\n".join(
        line.split("#", 1)[0] for line in _read(os.path.join(PKG, "env.py")).splitlines() if "os.environ" in line)))


def _names_in_table():
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    lines = text[text.index("## 7. Environment switches"):].splitlines()
    start = lines.index("| switch | default | read | selects |")
    names = []
    for row in lines[start + 2:]:
        if not row.startswith("|"):
            break
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert len(cells) == 4 and all(cells), row
        m = re.fullmatch(r"`(ALFI_[A-Z0-9_]+)`", cells[0])
        assert m, row
        names.append(m.group(1))
    assert len(names) == len(set(names))
    return set(names)


def test_header_module_and_table_list_the_same_switches():
    lib, pkg, table = _names_in_header(), _names_in_module(), _names_in_table()
    assert len(lib) == 10 and len(pkg) == 10 and not (lib & pkg)
    assert table == lib | pkg
    # every name is documented where it is read: in the comment of its accessor / the docstring of its function
    header = _read(os.path.join(CSRC, "env.h"))
    for name in lib:
        assert re.search(r"^// %s \(default " % name, header, re.M), name
    env = importlib.import_module("alfi_amd.env")
    documented = " ".join(fn.__doc__ or "" for fn in vars(env).values() if callable(fn))
    for name in pkg:
        assert name + " (default " in documented, name


def test_profiling_events_only_through_the_guard():
    """alfi_prof_begin / alfi_prof_end are folded into ProfScope: nothing in the library calls (or declares) them, and
    hipEventRecord on a profiling pair appears in the guard's two functions only."""
    for f in _csrc_files() + ["../../include/alfi_hip.h"]:
        text = _read(os.path.join(CSRC, f))
        assert not re.search(r"\balfi_prof_(begin|end)\b", text), f
        if f != "api_ctx.hip":
            assert "ev_pool[" not in text, f
    ctx = _read(os.path.join(CSRC, "api_ctx.hip"))
    guard = ctx[ctx.index("ProfScope::ProfScope("):ctx.index("// the sticky device-side error word")]
    assert guard.count("hipEventRecord(") == 2
    assert (ctx.count("hipEventRecord(ctx->ev_pool") + ctx.count("hipEventRecord(ctx_->ev_pool")) == 2
    common = _read(os.path.join(CSRC, "common.h"))
    assert "ProfScope(const ProfScope&) = delete;" in common and "~ProfScope() { close(); }" in common


# accessor, switch, what the inline expression of the previous revision gave with the variable unset, one setting, its value
CASES = [
    ("hip_lib", "ALFI_HIP_LIB", None, "/x/libalfi_hip.so", "/x/libalfi_hip.so"),            # os.environ.get(N) or <default path>
    ("host_threads", "ALFI_HOST_THREADS", 0, "5", 5),                                     # int(os.environ.get(N, "0")) or cpu_share()
    ("condense", "ALFI_CONDENSE", True, "0", False),                                      # os.environ.get(N, "1") != "0"
    ("coarse_sparse_min", "ALFI_COARSE_SPARSE_MIN", 8192, "100", 100),                    # int(os.environ.get(N, 8192))
    ("device_assembly", "ALFI_DEVICE_ASSEMBLY", True, "0", False),                        # os.environ.get(N, "1") != "0"
    ("macrostar_literal", "ALFI_MACROSTAR_LITERAL", False, "1", True),                    # os.environ.get(N) == "1"
    ("dist_transport", "ALFI_DIST_TRANSPORT", None, "callback", "callback"),              # os.environ.get(N) or <by backend>
    ("dist_overlap", "ALFI_DIST_OVERLAP", True, "0", False),                              # os.environ.get(N, "1") != "0"
    ("dist_overlap_min_dofs", "ALFI_DIST_OVERLAP_MIN_DOFS", None, "3000", 3000),          # int(os.environ[N]) if N in os.environ
    ("dist_global_generation", "ALFI_DIST_GLOBAL_GENERATION", False, "1", True),          # os.environ.get(N) == "1" (was: != "1", negated)
]


@pytest.fixture
def clean_env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("ALFI_"):
            monkeypatch.delenv(name)
    return monkeypatch


def test_cases_cover_every_accessor():
    env = importlib.import_module("alfi_amd.env")
    public = sorted(n for n, fn in vars(env).items() if callable(fn) and not n.startswith("_"))
    assert public == sorted(c[0] for c in CASES)
    assert {c[1] for c in CASES} == _names_in_module()


@pytest.mark.parametrize("fn,name,default,setting,value", CASES, ids=[c[1] for c in CASES])
def test_accessor_default_and_one_setting(clean_env, fn, name, default, setting, value):
    env = importlib.import_module("alfi_amd.env")
    got = getattr(env, fn)()
    assert got == default and type(got) is type(default)
    clean_env.setenv(name, setting)
    got = getattr(env, fn)()
    assert got == value and type(got) is type(value)


def test_comparisons_kept(clean_env):
    """!= "0" switches stay on for any other text, == "1" switches stay off for any other text; empty strings count as unset
    where the previous code used ``or``."""
    env = importlib.import_module("alfi_amd.env")
    for name, fn in (("ALFI_CONDENSE", env.condense), ("ALFI_DEVICE_ASSEMBLY", env.device_assembly), ("ALFI_DIST_OVERLAP", env.dist_overlap)):
        for text in ("1", "2", "", "off"):
            clean_env.setenv(name, text)
            assert fn() is True
    for name, fn in (("ALFI_MACROSTAR_LITERAL", env.macrostar_literal), ("ALFI_DIST_GLOBAL_GENERATION", env.dist_global_generation)):
        for text in ("0", "2", "", "on"):
            clean_env.setenv(name, text)
            assert fn() is False
    for name, fn in (("ALFI_HIP_LIB", env.hip_lib), ("ALFI_DIST_TRANSPORT", env.dist_transport)):
        clean_env.setenv(name, "")
        assert fn() is None


def test_env_module_is_standard_library_only():
    import ast
    tree = ast.parse(_read(os.path.join(PKG, "env.py")))
    imported = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    imported += [n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert imported == ["os"]
