"""GPRX_POISON reaches an allocation only through gprx_alloc.h (dev_malloc, dev_malloc_async): no
other file of the library may call the HIP device allocators, or its buffer silently escapes the
poisoned runs of the GPU suite (test_gpu_poison.py, test_gpu_lifecycle.py)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpr_amd", "csrc")
HELPER = "gprx_alloc.h"
ALLOC_CALL = re.compile(r"\b(hipMalloc|hipMallocAsync|hipExtMallocWithFlags|hipMallocManaged|hipMallocFromPoolAsync)\s*(<[^>]*>)?\s*\(")


def _code(text):
    """The file without its comments (string literals hold no calls)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return "\n".join(line.split("//", 1)[0] for line in text.splitlines())


def _calls(path):
    with open(path) as f:
        code = _code(f.read())
    return [(i + 1, m.group(1)) for i, line in enumerate(code.splitlines()) for m in ALLOC_CALL.finditer(line)]


def test_the_scan_sees_a_call_and_skips_a_comment(tmp_path):
    f = tmp_path / "x.hip"
    f.write_text("// hipMalloc(&p, 4) in a comment\nGPRX_HIP(hipMalloc(&p, b));\n"
                 "e = hipMallocAsync((void**)&q, b, s); /* hipMalloc( */\nhipExtMallocWithFlags (&p, b, f);\n"
                 "dev_malloc(&p, b); my_hipMalloc(&p);\n")
    assert _calls(str(f)) == [(2, "hipMalloc"), (3, "hipMallocAsync"), (4, "hipExtMallocWithFlags")]


def test_device_allocations_go_through_the_one_helper():
    files = sorted(n for n in os.listdir(CSRC) if n.endswith((".h", ".hip", ".cpp")))
    assert HELPER in files and len(files) > 20
    stray = {n: _calls(os.path.join(CSRC, n)) for n in files if n != HELPER}
    stray = {n: c for n, c in stray.items() if c}
    assert not stray, f"device allocations outside {HELPER} (file: [(line, call)]): {stray}"
    # the helper itself holds each allocator once
    assert sorted(c for _, c in _calls(os.path.join(CSRC, HELPER))) == ["hipExtMallocWithFlags", "hipMalloc", "hipMallocAsync"]
