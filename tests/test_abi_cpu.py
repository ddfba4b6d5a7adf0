"""CPU-only checks of the C ABI boundary (no GPU needed).

* librg_aead.so loads and exports every function include/rg_aead.h declares;
* the ctypes binding (rustyguard_amd/_lib.py) covers the same set;
* the public structs have the layout the header promises (compiled with gcc);
* without a GPU, rg_create fails cleanly with an error code (no crash), and
  the product package never falls back to a CPU path.
"""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import pytest

from conftest import REPO
from rustyguard_amd import _lib

HEADER = os.path.join(REPO, "include", "rg_aead.h")
TEST_HEADER = os.path.join(REPO, "include", "rg_aead_test.h")


def header_functions(path=HEADER):
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rg_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_batched_boundary():
    fns = header_functions()
    for must in ["rg_create", "rg_destroy", "rg_seal_batch_dev", "rg_open_batch_dev", "rg_seal_batch_host",
                 "rg_open_batch_host", "rg_chacha20poly1305_enc", "rg_chacha20poly1305_dec",
                 "rg_antireplay_would_accept", "rg_antireplay_mark_seen", "rg_send_batch", "rg_recv_batch"]:
        assert must in fns


def test_library_exports_every_header_symbol():
    path = _lib.lib_path()
    if not os.path.exists(path):
        from rustyguard_amd import build

        build.build()
    L = ctypes.CDLL(path)
    missing = [f for f in header_functions() if not hasattr(L, f)]
    assert not missing, missing
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rg_[a-z0-9_]+)", out))
    assert set(header_functions()) <= exported


def test_ctypes_binding_covers_header():
    assert set(header_functions()) == set(_lib.SIGNATURES), set(header_functions()) ^ set(_lib.SIGNATURES)


def _built():
    from rustyguard_amd import build

    build.build()
    return build


def _kernel_symbols(path):
    out = subprocess.run(["nm", "-C", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"(rg::(?:pipe_seal_kernel|pipe_open_kernel|tile_kernel|flat_kernel)<[^>]*>)", out))


def test_product_library_has_no_diagnostics_or_test_hooks():
    """the diagnostic seal modes (non-ciphertext output with a success status) and the stamp
    variants are not compiled into the product library -- only pipe_seal_kernel<0> and the unstamped tile
    kernels -- and the test hooks (include/rg_aead_test.h) are exported by the test library only."""
    b = _built()
    ks = _kernel_symbols(b.LIB)
    seals = {k for k in ks if k.startswith("rg::pipe_seal_kernel")}
    assert seals == {"rg::pipe_seal_kernel<0>"}, seals
    assert not any(k.startswith("rg::tile_kernel") and k.endswith(", true>") and k.count(",") == 2 for k in ks), ks
    prod = subprocess.run(["nm", "-D", "--defined-only", b.LIB], capture_output=True, text=True, check=True).stdout
    test = subprocess.run(["nm", "-D", "--defined-only", b.TEST_LIB], capture_output=True, text=True,
                          check=True).stdout
    hooks = header_functions(TEST_HEADER)
    assert hooks == ["rg_debug_fail_reserve", "rg_debug_last_wipe", "rg_debug_lose_completions",
                     "rg_debug_plan_handoff", "rg_debug_read_arena", "rg_debug_secret_state", "rg_debug_wait_selftest"]
    for h in hooks:
        assert f" T {h}\n" not in prod and f" T {h}\n" in test, h
    assert set(hooks) == set(_lib.TEST_SIGNATURES)
    # the test library carries the same kernels as the product one
    assert _kernel_symbols(b.TEST_LIB) == ks


def test_product_library_refuses_debug_modes(tmp_path):
    """rg_set_debug_mode(ctx, m != 0) and a stamp buffer are refused by the product library; checked on a
    context-free path here (a null context is refused first) and on a real context by the GPU tests."""
    L = _lib.lib()
    assert L.rg_set_debug_mode(None, 0) == -1  # null context
    src = open(os.path.join(REPO, "rustyguard_amd", "csrc", "rg_ctx.cpp")).read()
    body = src[src.index("int rg_set_debug_mode("):]
    body = body[:body.index("\n}\n")]
    assert "#if RG_DIAG" in body and 'mode != 0) return set_err(RG_EINVAL' in body


def test_abi_version():
    assert _lib.lib().rg_abi_version() == 6


def test_struct_layout_with_gcc(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rg_pkt_desc), offsetof(rg_pkt_desc, offset),
                   offsetof(rg_pkt_desc, len), offsetof(rg_pkt_desc, key_idx), sizeof(rg_antireplay),
                   offsetof(rg_antireplay, last));
            return 0;
        }
    """))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                   check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals == [16, 0, 8, 12, 33 * 8, 32 * 8]


def test_header_compiles_as_cxx(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "rg_aead.h"\nint main() { return rg_abi_version() == 1 ? 0 : 1; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                   check=True)


def test_create_without_gpu_fails_cleanly():
    """No silent CPU fallback: on a GPU-less host rg_create returns an error code."""
    code = textwrap.dedent(f"""
        import ctypes, sys
        sys.path.insert(0, {REPO!r})
        from rustyguard_amd import _lib
        h = ctypes.c_void_p()
        rc = _lib.lib().rg_create(0, ctypes.byref(h))
        print(rc, _lib.lib().rg_last_error().decode())
    """)
    env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", ""))
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("a GPU is present")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    rc = int(r.stdout.split()[0])
    assert rc < 0


def test_engine_raises_without_gpu():
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    from rustyguard_amd.aead import Engine
    from rustyguard_amd._lib import RgError

    with pytest.raises(RgError):
        Engine(0)


def test_product_package_does_not_import_oracle():
    pkg = os.path.join(REPO, "rustyguard_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(root, f)).read()
                assert "from oracle" not in text and "import oracle" not in text and "rg_oracle" not in text, f


def test_bounded_wait_loop_times_out_without_gpu():
    """every host wait of the library is the bounded polling loop (wait_bounded); the test
    library runs that loop against a fake completion (no HIP call).  A completion that never comes ends in
    RG_EDEVICE after the limit, not a hang; one that comes after k polls returns RG_OK after k + 1 polls."""
    L = _lib.lib_test()
    polls, ms = ctypes.c_uint32(), ctypes.c_uint32()
    rc = L.rg_debug_wait_selftest(60, 0xFFFFFFFF, ctypes.byref(polls), ctypes.byref(ms))
    assert rc == -2 and b"timed out" in L.rg_last_error()
    assert 60 <= ms.value < 2000 and polls.value > 10
    rc = L.rg_debug_wait_selftest(5000, 25, ctypes.byref(polls), ctypes.byref(ms))
    assert rc == 0 and polls.value == 26 and ms.value < 1000


def test_create_refuses_agent_scope_signals():
    """rg_create refuses ROC_SYSTEM_SCOPE_SIGNAL=0 (round 5: the host pipeline hung under it) before it
    touches the device, so the refusal shows without a GPU too."""
    code = textwrap.dedent(f"""
        import ctypes, sys
        sys.path.insert(0, {REPO!r})
        from rustyguard_amd import _lib
        h = ctypes.c_void_p()
        rc = _lib.lib().rg_create(0, ctypes.byref(h))
        print(rc, _lib.lib().rg_last_error().decode())
    """)
    env = dict(os.environ, ROC_SYSTEM_SCOPE_SIGNAL="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[0] == "-1" and "ROC_SYSTEM_SCOPE_SIGNAL" in r.stdout
