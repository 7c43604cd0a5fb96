"""The ctypes table of src/native.py against include/snvrag.h: every prototype and every structure.

native._SIGS and the Structure classes restate the header by hand; a wrong argument type there sends
a wrong pointer to a kernel.  The header is regular enough for a regular-expression reader (below):
comments and preprocessor lines stripped, then `typedef struct { ... } name_t;` and `snvrag_*(...)`
prototypes.  Needs no GPU and no built library.
"""
import copy
import ctypes as C
import re
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "rag-snvbert_amd"))
from src import native  # noqa: E402

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "size_t": C.c_size_t,
           "uint64_t": C.c_uint64}
STRUCTS = {"snvrag_epilogue_t": native.Epilogue, "snvrag_rownorm_t": native.RowNormS,
           "snvrag_ln_post_t": native.LnPost, "snvrag_posfeat_w_t": native.PosfeatW,
           "snvrag_afgate_w_t": native.AfGateW, "snvrag_gt_w_t": native.GtW, "snvrag_layer_t": native.LayerW,
           "snvrag_derive_job_t": native.DeriveJob, "snvrag_adam_t": native.AdamS,
           "snvrag_feature_tables_t": native.FeatureTables}
# snvrag_derive takes the job table's DEVICE address (kernels.derive_table uploads the packed
# DeriveJob array), so Python passes it as a plain address, not POINTER(DeriveJob)
UNTYPED_STRUCT_PTR = {("snvrag_derive", 0)}


# ---------------------------------------------------------------- the header reader
def _c_type(text):
    """'const float* const' -> ('float', 1): base type name and pointer depth."""
    depth = text.count("*")
    words = [w for w in text.replace("*", " ").split() if w != "const"]
    assert len(words) == 1, f"unreadable type {text!r}"
    return words[0], depth


def parse_header(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*?(?<!\\)$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    structs = {}

    def struct(m):
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            first, *more = [d.strip() for d in decl.split(",")]
            fm = re.fullmatch(r"(.*?)(\w+)\s*(?:\[(\d+)\])?", first)
            base, depth = _c_type(fm.group(1))
            fields.append((fm.group(2), base, depth, int(fm.group(3) or 0)))
            for d in more:                       # comma declarators share the base type
                dm = re.fullmatch(r"(\**)\s*(\w+)\s*(?:\[(\d+)\])?", d)
                fields.append((dm.group(2), base, len(dm.group(1)), int(dm.group(3) or 0)))
        structs[m.group(2)] = fields
        return " "

    text = re.sub(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    funcs = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(snvrag_\w+)\s*\(([^()]*)\)\s*;", text):
        args = []
        body = m.group(3).strip()
        if body and body != "void":
            for a in body.split(","):
                am = re.fullmatch(r"(.*?[\s\*])(\w+)", a.strip())   # the last word is the name
                args.append(_c_type(am.group(1)))
        funcs[m.group(2)] = (args, _c_type(m.group(1)))
    return structs, funcs


HEADER_STRUCTS, HEADER_FUNCS = parse_header((REPO / "include" / "snvrag.h").read_text())


# ---------------------------------------------------------------- the comparison
def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def _type_error(ctype, py, where, struct_map):
    """None when the ctypes type ``py`` matches the C type (base, pointer depth)."""
    base, depth = ctype
    if depth == 0:
        if base == "void":
            return None if py is None else f"{where}: void, Python has {py}"
        want = SCALARS.get(base)
        if want is None:
            return f"{where}: C type {base} is not a known scalar"
        return None if py is want else f"{where}: C {base}, Python {py}"
    if not _is_pointer(py):
        return f"{where}: C {base}{'*' * depth}, Python {py} is not a pointer"
    if base == "char" and depth == 1:
        return None if py is C.c_char_p else f"{where}: const char* must be c_char_p, Python {py}"
    if base in struct_map and depth == 1 and where not in UNTYPED_STRUCT_PTR_NAMES:
        return None if py is C.POINTER(struct_map[base]) else f"{where}: must be POINTER({struct_map[base].__name__})"
    if py is C.c_char_p:
        return f"{where}: c_char_p for a C {base}*"
    return None                                  # c_void_p or a typed data pointer: one address either way


UNTYPED_STRUCT_PTR_NAMES = {f"{f} arg {i}" for f, i in UNTYPED_STRUCT_PTR}


def sig_errors(sigs, funcs=HEADER_FUNCS, struct_map=STRUCTS):
    errs = []
    for name in sorted(set(funcs) | set(sigs)):
        if name not in sigs or name not in funcs:
            errs.append(f"{name}: only in {'the header' if name in funcs else 'native._SIGS'}")
            continue
        (cargs, cres), (pargs, pres) = funcs[name], sigs[name]
        if len(cargs) != len(pargs):
            errs.append(f"{name}: {len(cargs)} arguments in the header, {len(pargs)} in Python")
            continue
        checks = [(c, p, f"{name} arg {i}") for i, (c, p) in enumerate(zip(cargs, pargs))] + [(cres, pres, f"{name} result")]
        errs += [e for e in (_type_error(c, p, w, struct_map) for c, p, w in checks) if e]
    return errs


def struct_errors(struct_map, structs=HEADER_STRUCTS):
    errs = [f"{n}: only in {'the header' if n in structs else 'the test table'}"
            for n in sorted(set(structs) ^ set(struct_map))]
    for name in sorted(set(structs) & set(struct_map)):
        cf, pf = structs[name], struct_map[name]._fields_
        if [f[0] for f in cf] != [f[0] for f in pf]:
            errs.append(f"{name}: fields {[f[0] for f in cf]} in the header, {[f[0] for f in pf]} in Python")
            continue
        for (fname, base, depth, alen), (_, py) in zip(cf, pf):
            plen = 0
            if isinstance(py, type) and issubclass(py, C.Array):
                plen, py = py._length_, py._type_
            if plen != alen:
                errs.append(f"{name}.{fname}: array length {alen} in the header, {plen} in Python")
            e = _type_error((base, depth), py, f"{name}.{fname}", struct_map)
            if e:
                errs.append(e)
    return errs


# ---------------------------------------------------------------- the tests
def test_header_reader_sees_everything():
    # the reader itself: every exported name, every structure, comma declarators and [4] arrays
    assert set(HEADER_FUNCS) == set(native._SIGS)
    assert len(HEADER_FUNCS) >= 122 and len(HEADER_STRUCTS) == 10
    job = {f[0]: f for f in HEADER_STRUCTS["snvrag_derive_job_t"]}
    assert job["nparts"] == ("nparts", "int32_t", 0, 0)
    assert job["cs"] == ("cs", "int64_t", 0, 4)
    assert job["src"] == ("src", "float", 1, 4)
    assert HEADER_FUNCS["snvrag_last_error"] == ([], ("char", 1))
    assert HEADER_FUNCS["snvrag_derive"][0][0] == ("snvrag_derive_job_t", 1)


def test_signatures_match_the_header():
    assert sig_errors(native._SIGS) == []


def test_structures_match_the_header():
    assert struct_errors(STRUCTS) == []


def test_abi_version_is_unchanged():
    assert native.ABI_VERSION == 31


def _mutated_structs(name, i, j):
    fields = list(STRUCTS[name]._fields_)
    fields[i], fields[j] = fields[j], fields[i]
    return dict(STRUCTS, **{name: type(name, (C.Structure,), {"_fields_": fields})})


@pytest.mark.parametrize("case", ["i64_as_int", "dropped_argument", "swapped_fields"])
def test_check_rejects_a_mutated_table(case):
    sigs = copy.deepcopy(dict(native._SIGS))
    if case == "i64_as_int":
        args, res = sigs["snvrag_tail_forward"]
        assert args[0] is C.c_int64
        sigs["snvrag_tail_forward"] = ([C.c_int] + args[1:], res)
        assert sig_errors(sigs) == ["snvrag_tail_forward arg 0: C int64_t, Python <class 'ctypes.c_int'>"]
    elif case == "dropped_argument":
        args, res = sigs["snvrag_knn_scan"]
        sigs["snvrag_knn_scan"] = (args[:-1], res)
        assert sig_errors(sigs) == ["snvrag_knn_scan: 13 arguments in the header, 12 in Python"]
    else:
        # rows <-> kind of the derive job: same sizes elsewhere, different names and kinds
        errs = struct_errors(_mutated_structs("snvrag_derive_job_t", 0, 2))
        assert len(errs) == 1 and errs[0].startswith("snvrag_derive_job_t: fields ")
        # and two fields of one name set but different kinds (a pointer and a float)
        lw = native.LayerW._fields_
        i, j = [n for n, _ in lw].index("c2g"), [n for n, _ in lw].index("q_scale")
        bad = list(lw)
        bad[i], bad[j] = (lw[i][0], lw[j][1]), (lw[j][0], lw[i][1])
        errs = struct_errors(dict(STRUCTS, snvrag_layer_t=type("L", (C.Structure,), {"_fields_": bad})))
        assert len(errs) == 2 and all(e.startswith("snvrag_layer_t.") for e in errs)
