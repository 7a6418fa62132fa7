"""The workspace types of the host drivers (csrc/krylov_ws.h) and where their memory is freed.  CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alfi_amd", "csrc")

# members that are Krylov arrays or block buffers of a level or a saddle
WS_MEMBER = re.compile(r"(->|\.)(V|Z|w|hs|p)\b|blk_(stage|ctmp|carry|part|mg_[bxr]|tmp_u|ws|V|Z|w|hs)\b")
RELEASES = ("krylov_ws_release", "slot_buf_release")
# who may call a release: the two types' own ensure / resize, and the lifetime functions
RELEASE_CALLERS = {"krylov_ws_ensure", "slot_buf_resize", "block_release_patch_buffers", "release_workspaces"}


def _sources(ext):
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(ext)}


def _function_of(text, pos):
    """name of the function whose body holds text[pos] (the last definition at column 0 before it)"""
    found = None
    for m in re.finditer(r"^(?:static |inline )*[\w:<>\*&]+[ \*&]+(\w+)\([^;{]*\) \{$", text[:pos], re.M | re.S):
        found = m.group(1)
    return found


def test_layout_and_grow_rule_under_host_sanitizers(tmp_path):
    """tests/krylov_ws_check.cpp: every accessor against the long-hand formula, first and last entry of every vector written,
    no two regions overlap; the slot buffer's grow rule against block_slots_needed"""
    exe = str(tmp_path / "krylov_ws_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "krylov_ws_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout


def test_workspaces_are_freed_in_one_place():
    """no dev_free of a Krylov array or a block buffer outside the two types' release functions (api_block.hip), and nobody
    calls those but the types' ensure / resize and the lifetime functions"""
    hips = _sources(".hip")
    frees, calls = [], []
    for name, text in hips.items():
        for m in re.finditer(r"dev_free\(([^;]*)\);", text):
            if WS_MEMBER.search(m.group(1)) and "blk_dofs" not in m.group(1):
                frees.append((name, _function_of(text, m.start()), m.group(1)))
        for m in re.finditer(r"\b(%s)\(" % "|".join(RELEASES), text):
            line = text[text.rfind("\n", 0, m.start()) + 1:m.start()]
            if line.strip() != "void":                            # (not the definition itself)
                calls.append((name, _function_of(text, m.start())))
    assert frees and all(f[0] == "api_block.hip" and f[1] in RELEASES for f in frees), frees
    assert {f[2] for f in frees} == {"ws->V", "ws->Z", "ws->w", "ws->hs", "buf->p"}, frees
    assert calls and all(c[0] == "api_block.hip" and c[1] in RELEASE_CALLERS for c in calls), calls
    # the lifetime functions are called from where a patch set is replaced and from the two destroy functions, and nowhere else
    users = {name: sorted(set(re.findall(r"\b(block_release_patch_buffers|release_workspaces)\(", text)))
             for name, text in hips.items() if name != "api_block.hip"}
    users = {k: v for k, v in users.items() if v}
    assert users == {"api_level.hip": ["release_workspaces"], "api_patches.hip": ["block_release_patch_buffers"],
                     "api_saddle.hip": ["release_workspaces"]}, users


def test_slot_stride_arithmetic_is_in_the_header_only():
    """(K + 1) * ldv, K * ldv between slots, HsLayout(K).total per slot: krylov_ws.h and no other file of csrc"""
    stride = re.compile(r"\(\s*(?:\(int64_t\))?\s*\(?\s*\w*(?:K|kmax|restart)\s*\+\s*1\s*\)\s*\*\s*[\w.>-]*ldv")
    holders = [f for f, text in {**_sources(".hip"), **_sources(".h"), **_sources(".cpp")}.items()
               if any(stride.search(ln) for ln in text.split("\n") if not ln.lstrip().startswith("//"))]
    assert holders == ["krylov_ws.h"], holders
    header = open(os.path.join(CSRC, "krylov_ws.h")).read()
    assert "int64_t vs() const { return (int64_t)(K + 1) * ldv; }" in header
    assert "int64_t zs() const { return (int64_t)K * ldv; }" in header
    assert "int64_t hstride() const { return HsLayout(K).total; }" in header
    assert "#include <hip" not in header and "hip_runtime" not in header
