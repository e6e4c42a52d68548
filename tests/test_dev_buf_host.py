"""Device memory of libcorahip.so has one owner, dev_buf (cora_amd/csrc/dev_buf.h): the library's sources allocate and
free through it alone, and the type itself is tested by a stand-alone host program under the address and
undefined-behaviour sanitizers (cora_amd/csrc/tools/dev_buf_test.cpp, no GPU and no HIP runtime)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cora_amd", "csrc")


def _sources():
    """name -> text of every source of the library (tools/ holds stand-alone probes, not library code)"""
    out = {}
    for pat in ("*.hip", "*.h", "*.inc"):
        for path in glob.glob(os.path.join(CSRC, pat)):
            out[os.path.basename(path)] = open(path).read()
    assert "dev_buf.h" in out and "ctx.hip" in out and len(out) > 40
    return out


def _function_body(text, name):
    """the braces of the definition of `name` (first `name(...) {` in text), by brace counting"""
    m = re.search(r"\b%s\s*\([^;{]*\)\s*\{" % re.escape(name), text)
    assert m, name
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def _calls_outside(call, entry_point):
    """(file, line) of every `call(` outside dev_buf.h and the body of the C ABI's `entry_point` in ctx.hip"""
    found = []
    for name, text in _sources().items():
        if name == "dev_buf.h":
            continue
        if name == "ctx.hip":
            body = _function_body(text, entry_point)
            assert body.count(call + "(") == 1
            text = text.replace(body, "\n" * body.count("\n"))
        found += [(name, n + 1) for n, line in enumerate(text.split("\n")) if call + "(" in line]
    return found


def test_hipfree_only_in_dev_buf_and_corahip_free():
    assert "hipFree(" in _sources()["dev_buf.h"]
    assert _calls_outside("hipFree", "corahip_free") == []


def test_hipmalloc_only_in_dev_buf_and_corahip_malloc():
    assert "hipMalloc(" in _sources()["dev_buf.h"]
    assert _calls_outside("hipMalloc", "corahip_malloc") == []


def test_dev_mem_is_gone():
    assert [n for n, t in _sources().items() if re.search(r"struct\s+dev_mem\b", t)] == []


def test_plan_destroy_frees_no_member():
    body = _function_body(_sources()["sht_plan.hip"], "corahip_sht_plan_destroy")
    assert "delete p" in body
    assert "->" not in body and "hipFree" not in body and "reset" not in body, body


def test_dev_buf_header_needs_only_the_runtime_api():
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", _sources()["dev_buf.h"])
    assert [i for i in includes if i.startswith("hip/")] == ["hip/hip_runtime_api.h"]
    assert all(i.startswith("hip/") or "." not in i for i in includes), includes   # besides it, the C++ library only


def test_dev_buf_program_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler (g++)")
    # the Makefile's own rule (build, then run), with the program written outside the source tree
    r = subprocess.run(["make", "-s", "-C", CSRC, "devbuftest", "HOSTCXX=" + cxx, "DEVBUF_TEST=" + str(tmp_path / "dev_buf_test")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "dev_buf_test OK" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
