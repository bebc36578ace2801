"""Test infrastructure: include/slk.h parsed into declarations, and the refusal sweep of tests/test_abi.py.

`declarations()` strips the comments and returns every `slk_*` declaration with its parameters' types and names.

Run as a script, this file calls every entry that takes a pointer with arguments that must be refused before a launch
and prints one JSON object {entry: {form: status}}. It is meant for a child process to which no GPU is visible and
calls nothing if it sees one (exit status 3): if a check were missing the launch then fails (hipErrorNoDevice) instead
of running a kernel on null pointers. Forms, per entry:
  minus     every int / int64_t at -1, every pointer null
  null      every int at 1 (ONES where 1 is not a legal value), every pointer null
  zero      every int at 0, every pointer null
  dummy     every int at 1, every pointer a distinct non-null dummy (16-byte aligned, never dereferenced by host code)
  -<name>   as dummy, but the pointer <name> null
Arrays the header calls host memory are real host arrays (their elements dummies), since the entry reads them;
unsigned arguments are 0, floats and doubles 0.5."""
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CTYPE_OF = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint, "int64_t": ctypes.c_int64,
            "float": ctypes.c_float, "double": ctypes.c_double}

# where 1 is not a legal value of an int: the image entries take (C, H, W) = (1, 28, 28) or (3, 32, 32)
ONES = {"C": 1, "H": 28, "W": 28, "pad": 0, "flip_enabled": 0}
HOST_INT_ARRAYS = ("nslab", "n", "group", "nw")       # `const int*` of the *_multi entries: host arrays of nseg ints
HOST_FLOAT_ARRAYS = ("mean", "std")                   # slk_image_batch*: host arrays of C floats


def declarations(path=os.path.join(ROOT, "include", "slk.h")):
    """[(return type, name, [(parameter type, parameter name)])], in the header's order."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    out = []
    for ret, name, plist in re.findall(r"\b(const\s+char\s*\*|int64_t|int)\s+(slk_\w+)\s*\(([^)]*)\)\s*;", src):
        params = []
        for p in plist.split(","):
            p = " ".join(p.split())
            if p in ("", "void"):
                continue
            m = re.match(r"(.*?)(\w+)$", p)
            params.append((m.group(1).strip(), m.group(2)))
        out.append((" ".join(ret.split()), name, params))
    return out


def param_ctype(ptype):
    """The ctypes class of a parameter type: any pointer is c_void_p, scalars by CTYPE_OF (KeyError: unknown)."""
    if "*" in ptype:
        return ctypes.c_void_p
    return CTYPE_OF[ptype.replace("const ", "").strip()]


def host_kind(entry, ptype, pname):
    """"pointers" / "ints" / "floats" for a parameter that is a host array, else None."""
    if re.search(r"\*\s*const\s*\*", ptype):
        return "pointers"
    if ptype.replace(" ", "") == "constint*" and pname in HOST_INT_ARRAYS and "_multi" in entry:
        return "ints"
    if pname in HOST_FLOAT_ARRAYS and entry.startswith("slk_image_batch"):
        return "floats"
    return None


def pointer_params(params):
    return [n for t, n in params if "*" in t and n != "stream"]


_keep = []


def _dummy(entry, i, ptype, pname):
    base = 0x100000 * (i + 1)
    kind = host_kind(entry, ptype, pname)
    if kind is None:
        return base
    if kind == "pointers":
        arr = (ctypes.c_void_p * 8)(*[base + 0x10000 * j for j in range(8)])
    elif kind == "ints":
        arr = (ctypes.c_int * 8)(*([0] * 8 if pname == "group" else [1] * 8))
    else:
        arr = (ctypes.c_float * 8)(*[0.5] * 8)
    _keep.append(arr)
    return ctypes.cast(arr, ctypes.c_void_p)


def arguments(entry, params, count, pointers, null=None):
    args = []
    for i, (t, n) in enumerate(params):
        if "*" in t:
            args.append(_dummy(entry, i, t, n) if pointers and n != null and n != "stream" else None)
        elif t in ("int", "int64_t"):
            args.append(ONES.get(n, 1) if count == 1 else count)
        elif t in ("unsigned", "uint32_t"):
            args.append(0)
        else:
            args.append(0.5)
    return args


def sweep():
    sys.path.insert(0, os.path.join(ROOT, "split-learning-k8s_amd"))
    import torch
    if torch.cuda.is_available():
        print("a GPU is visible: the sweep is not run", file=sys.stderr)
        return 3
    from splitcnn import _lib
    lib = _lib.load()
    out = {}
    for _, entry, params in declarations():
        ptrs = pointer_params(params)
        if not ptrs:
            continue
        fn = getattr(lib, entry)
        res = {"minus": fn(*arguments(entry, params, -1, False)), "null": fn(*arguments(entry, params, 1, False)),
               "zero": fn(*arguments(entry, params, 0, False)), "dummy": fn(*arguments(entry, params, 1, True))}
        for name in ptrs:
            res["-" + name] = fn(*arguments(entry, params, 1, True, null=name))
        out[entry] = res
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(sweep())
