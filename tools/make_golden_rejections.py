#!/usr/bin/env python3
"""Generate tests/golden/capi_rejections_abi37.json: what every streamed entry point of the C-ABI (an scr_* function of
include/splatco_raster.h whose last parameter is `void* stream`) answers to a few synthetic argument vectors that it must
turn down, or accept as empty input, BEFORE it launches anything.  tests/test_capi_rejections_host.py replays the table:
an argument check that a later change loses, reorders or rewords shows up there, on a machine without a device.

Run it on a machine WITHOUT a device, against the build whose behaviour is the reference (the parent commit's, when the
entry points are being moved): with a device, a vector that passes the checks becomes a launch on made-up pointers.

A vector is "<pointers>_<integer>": every pointer parameter NULL ("null") or the address of one zeroed, 4096-byte
aligned host buffer of 4096 bytes ("buf": host arrays, structs and tables of pointers then read as zeros), every integer
parameter the given value, every float 0.5, the stream NULL.  Kept: the cases that came back before a launch -- a
non-zero status whose message neither begins with "launch of" nor contains "failed:" (both are HIP's verdict on an
enqueue), or status 0 (empty input).  The other cases reached the runtime; they are printed, not recorded.

The table only grows.  tests/golden/capi_rejections.json (BASE) is the table as it was first recorded, at ABI 36, and stays
as it is; OUT holds BASE's rows, unchanged and in place, with the rows of the entry points added since (ABI 37:
scr_filter3d_*) among them in header order.  main() refuses to write a table that loses or changes a row of BASE, and
tests/test_filter3d_host.py checks the same of the committed file.
"""
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = os.path.join(ROOT, "tests", "golden", "capi_rejections.json")
OUT = os.path.join(ROOT, "tests", "golden", "capi_rejections_abi37.json")
VECTORS = ("null_1", "null_-1", "null_0", "buf_1", "buf_-1", "buf_0")
BUF_BYTES = 4096


def streamed_entry_points():
    """Names of the header's functions whose last parameter is `void* stream`, in header order."""
    hdr = open(os.path.join(ROOT, "include", "splatco_raster.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    hdr = re.sub(r"^\s*#[^\n]*", "", hdr, flags=re.M)
    hdr = re.sub(r"typedef\s+struct.*?\}\s*\w+\s*;|\benum\s*\{.*?\}\s*;", "", hdr, flags=re.S)
    protos = re.findall(r"\b(scr_\w+)\s*\(([^()]*)\)\s*;", hdr)
    return [name for name, params in protos if "".join(params.split(",")[-1].split()) == "void*stream"]


class Buffer:
    """One zeroed host buffer at a 4096-byte boundary (alignment checks see the same address bits everywhere)."""

    def __init__(self):
        self.raw = C.create_string_buffer(2 * BUF_BYTES)
        self.address = (C.addressof(self.raw) + BUF_BYTES - 1) // BUF_BYTES * BUF_BYTES

    def clear(self):
        C.memset(self.address, 0, BUF_BYTES)


def arguments(argtypes, vector, buf):
    """The argument list of `vector` for a streamed function with these ctypes argtypes (the stream, last, is NULL)."""
    pointers, integer = vector.split("_")
    args = []
    for t in argtypes[:-1]:
        if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
            args.append(None if pointers == "null" else C.cast(buf.address, t))
        elif t in (C.c_float, C.c_double):
            args.append(0.5)
        else:
            args.append(int(integer))
    return args + [None]


def run_case(_C, name, vector, buf):
    """(status, message) of one call; the message is "" for status 0 (scr_last_error keeps the previous failure's text)."""
    sig = next(s for s in _C.SIGNATURES if s[0] == name)
    buf.clear()
    rc = getattr(_C.lib, name)(*arguments(sig[2:], vector, buf))
    return rc, ("" if rc == 0 else _C.lib.scr_last_error().decode())


def before_launch(rc, message):
    return rc == 0 or not (message.startswith("launch of") or "failed:" in message)


def added_rows(base, table):
    """The rows of `table` that are not rows of `base`; AssertionError unless `table` holds every row of `base`, unchanged
    and in the same order (the table only grows)."""
    it = iter(table)
    extra = []
    for row in base:
        for got in it:
            if got == row:
                break
            extra.append(got)
        else:
            raise AssertionError(f"the table lost or changed the recorded row {row}")
    return extra + list(it)


def main():
    sys.path.insert(0, ROOT)
    import torch
    if torch.cuda.is_available():
        sys.exit("a device is present: run this on a machine without one (see the module docstring)")
    from splatco_amd import _C
    buf = Buffer()
    kept, dropped = [], []
    for name in streamed_entry_points():
        for vector in VECTORS:
            rc, message = run_case(_C, name, vector, buf)
            row = {"name": name, "vector": vector, "rc": rc, "error": message}
            (kept if before_launch(rc, message) else dropped).append(row)
    for row in dropped:
        print("dropped (reached the runtime):", row["name"], row["vector"], row["rc"], row["error"])
    missing = sorted(set(streamed_entry_points()) - {r["name"] for r in kept})
    assert not missing, f"no case of {missing} returns before a launch"
    with open(BASE) as f:
        new = added_rows(json.load(f), kept)
    print(f"{len(new)} rows beyond {BASE}: {sorted({r['name'] for r in new})}")
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in kept) + "\n]\n")
    print(f"{OUT}: {len(kept)} cases kept, {len(dropped)} dropped, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
