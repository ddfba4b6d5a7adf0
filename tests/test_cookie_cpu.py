"""CPU-only checks of the under-load handshake filter's boundary (rg_cookie_reply_batch_dev): the public
structs' layout, the source-address encoding, the integration document and the exported symbol."""
import os
import re
import subprocess
import textwrap

from conftest import REPO
from rustyguard_amd import aead

HEADER_DIR = os.path.join(REPO, "include")


def test_cookie_structs_layout_with_gcc(tmp_path):
    src = tmp_path / "cookie_layout.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "rg_aead.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(rg_cookie_keys), offsetof(rg_cookie_keys, mac1_key),
                   offsetof(rg_cookie_keys, cookie_key), offsetof(rg_cookie_keys, secret), sizeof(rg_src_addr),
                   offsetof(rg_src_addr, port_le), offsetof(rg_src_addr, pad), (int)RG_PKT_COOKIE, RG_ABI_VERSION);
            return 0;
        }
    """))
    exe = tmp_path / "cookie_layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals == [96, 0, 32, 64, 24, 16, 18, 7, 6]
    assert aead.PKT_COOKIE == 7


def test_encode_src_addr_follows_new_cookie():
    """CookieState::new_cookie (rustyguard-crypto/src/lib.rs:95-103): a[..4] or a[..16] = the IP's octets,
    a[16..18] = the port little-endian; rg_src_addr pads that to 24 bytes."""
    a = aead.encode_src_addr("192.0.2.7", 51820)
    assert a == bytes([192, 0, 2, 7]) + bytes(12) + bytes([0x6C, 0xCA]) + bytes(6) and len(a) == 24
    b = aead.encode_src_addr("2001:db8::1:2", 1)
    assert b == bytes.fromhex("20010db8000000000000000000010002") + bytes([1, 0]) + bytes(6)
    assert aead.encode_src_addr("0.0.0.0", 65535)[16:18] == b"\xff\xff"
    for bad in (-1, 65536):
        try:
            aead.encode_src_addr("192.0.2.7", bad)
        except ValueError:
            continue
        raise AssertionError(f"port {bad} accepted")


def test_integration_document_names_the_entry_point():
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    blocks = re.findall(r'extern "C" \{.*?\n\}', text, flags=re.S)
    assert blocks and any("rg_cookie_reply_batch_dev" in b and "rg_cookie_keys" in b and "rg_src_addr" in b
                          for b in blocks)


def test_both_libraries_export_the_symbol():
    from rustyguard_amd import build

    build.build()
    for lib in (build.LIB, build.TEST_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        assert " T rg_cookie_reply_batch_dev\n" in out, lib
