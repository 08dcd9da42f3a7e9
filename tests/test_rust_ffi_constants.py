"""The constants of integration/rust/ffi.rs carry the header's values and signedness, not only its
names: every `#define BJ_*` of include/boojum_mi355x.h, read here with C's literal rules
(decimal or hexadecimal, a `u` suffix is unsigned), equals the `pub const` of the same name."""
import os
import re

from test_abi import ROOT


def header_defines():
    text = open(os.path.join(ROOT, "include", "boojum_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, body in re.findall(r"^#define (BJ_[A-Z0-9_]+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        body = body.strip("()")
        if body == "UINT64_MAX":
            out[name] = ((1 << 64) - 1, "u64")
            continue
        unsigned = body[-1] in "uU"
        out[name] = (int(body.rstrip("uU"), 0), "u32" if unsigned else "c_int")
    return out


def rust_consts():
    text = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    out = {}
    for name, ty, val in re.findall(r"^pub const (BJ_[A-Z0-9_]+): (\w+) = ([^;]+);", text, flags=re.M):
        out[name] = ((1 << 64) - 1 if val == "u64::MAX" else int(val, 0), ty)
    return out


def test_every_define_keeps_its_value_and_type():
    want, got = header_defines(), rust_consts()
    assert want and got == want


def test_gate_check_begin_is_the_top_bit_of_a_u32():
    assert rust_consts()["BJ_GATE_CHECK_BEGIN"] == (0x80000000, "u32")
    from boojum_amd import gates
    assert gates.CHECK_BEGIN == header_defines()["BJ_GATE_CHECK_BEGIN"][0]
