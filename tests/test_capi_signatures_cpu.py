"""CPU-only: the ctypes signature of every function of the loaded library agrees with its prototype in
include/carma_mi355.h -- arity, exact scalar types, pointer kinds and the return type.  tests/test_capi_symbols.py holds the
NAMES to the header; this holds what a wrong `c_int` against a `long` would otherwise turn into stack garbage on a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"int": C.c_int, "long": C.c_long, "double": C.c_double, "uint64_t": C.c_uint64, "unsigned": C.c_uint,
           "unsigned long long": C.c_ulonglong}
# what a typed POINTER(T) may point at, by the C pointee; every other pointee (an opaque handle, void, char) is untyped
POINTEES = {"double": C.c_double, "int": C.c_int, "long": C.c_long, "unsigned long long": C.c_ulonglong}
UNTYPED = (C.c_void_p, C.c_char_p)


def _c_type(text):
    """'const double* time' -> ('double', 1); 'carma_ctx* const* hs' -> ('carma_ctx', 2); 'unsigned long long iter' -> (.., 0)."""
    stars = text.count("*")
    words = [w for w in text.replace("*", " ").split() if w != "const"]
    return " ".join(words), stars


def prototypes():
    """{name: (return type, [parameter types])} of every `ret carma_x(args);` of the header, each type as _c_type gives it."""
    txt = open(os.path.join(ROOT, "include", "carma_mi355.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(carma_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = []
        if " ".join(args.split()) != "void":
            for a in args.split(","):
                a = a.strip()
                if not a.endswith("*"):                        # drop the parameter's name
                    a = re.sub(r"\b\w+$", "", a)
                params.append(_c_type(a))
        assert name not in out, "%s is declared twice" % name
        out[name] = (_c_type(ret), params)
    return out


def _param_ok(ctype, base, stars):
    if stars == 0:
        return ctype is SCALARS.get(base)
    if ctype in UNTYPED:
        return True
    pointee = C.c_void_p if stars == 2 else POINTEES.get(base)     # T* const*: an array of untyped pointers
    return pointee is not None and ctype is C.POINTER(pointee)


def _ret_ok(restype, base, stars):
    if stars:
        return restype in UNTYPED
    return restype is (None if base == "void" else SCALARS.get(base))


def mismatches(name, proto, restype, argtypes):
    """The disagreements of one ctypes signature with its prototype, as a list of strings (empty: they agree)."""
    (rbase, rstars), params = proto
    bad = []
    if not _ret_ok(restype, rbase, rstars):
        bad.append("%s: returns %s%s, restype is %r" % (name, rbase, "*" * rstars, restype))
    if argtypes is None:
        if params:
            bad.append("%s: takes %d arguments and has no argtypes" % (name, len(params)))
        return bad
    if len(argtypes) != len(params):
        return bad + ["%s: takes %d arguments, argtypes has %d" % (name, len(params), len(argtypes))]
    for i, (ct, (base, stars)) in enumerate(zip(argtypes, params)):
        if not _param_ok(ct, base, stars):
            bad.append("%s: argument %d is %s%s, argtypes has %r" % (name, i, base, "*" * stars, ct))
    return bad


def test_header_is_read_whole():
    protos = prototypes()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "carma_mi355.h")).read(), flags=re.S)
    assert sorted(protos) == sorted(set(re.findall(r"\b(carma_[a-z0-9_]+)\s*\(", txt)))    # as tests/test_capi_symbols.py reads it
    assert protos["carma_version"] == (("char", 1), [])
    assert protos["carma_pt_iterate"] == (("int", 0), [("carma_ctx", 1), ("long", 0), ("int", 0)])
    assert protos["carma_pt_iterate_sharded"][1][0] == ("carma_ctx", 2)
    assert ("unsigned long long", 0) in protos["carma_pt_debug_draws"][1]
    assert sum(not p for _, p in protos.values()) >= 3          # the (void) ones


def test_every_signature_agrees_with_the_header():
    import carma_pack_amd._lib as L
    bad = []
    for name, proto in sorted(prototypes().items()):
        fn = getattr(L.lib, name)
        bad += mismatches(name, proto, fn.restype, fn.argtypes)   # (no argtypes at all passes for a (void) prototype only)
    assert not bad, "\n".join(bad)


def test_comparison_reports_a_wrong_scalar_a_wrong_pointer_and_a_wrong_arity():
    """Negative control: the comparison is not vacuous."""
    import carma_pack_amd._lib as L
    protos = prototypes()
    fn = L.lib.carma_pt_iterate
    good = list(fn.argtypes)
    assert C.c_long in good and mismatches("carma_pt_iterate", protos["carma_pt_iterate"], fn.restype, good) == []
    swapped = [C.c_int if t is C.c_long else t for t in good]
    rep = mismatches("carma_pt_iterate", protos["carma_pt_iterate"], fn.restype, swapped)
    assert len(rep) == 1 and "argument 1 is long" in rep[0], rep
    assert mismatches("carma_pt_iterate", protos["carma_pt_iterate"], fn.restype, good[:-1])
    assert mismatches("carma_pt_iterate", protos["carma_pt_iterate"], C.c_long, good)
    assert mismatches("carma_pt_iterate", protos["carma_pt_iterate"], fn.restype, None)
    fn = L.lib.carma_mctx_create                                 # (..., const long* offsets, ...): POINTER(c_int) is wrong, c_void_p is not
    good = list(fn.argtypes)
    i = protos["carma_mctx_create"][1].index(("long", 1))
    for ct, ok in ((C.POINTER(C.c_int), False), (C.POINTER(C.c_long), True), (C.c_void_p, True), (C.c_long, False)):
        rep = mismatches("carma_mctx_create", protos["carma_mctx_create"], fn.restype, good[:i] + [ct] + good[i + 1:])
        assert (rep == []) == ok, (ct, rep)
    assert mismatches("carma_pt_iterations_done", protos["carma_pt_iterations_done"], C.c_int, [C.c_void_p])
    assert mismatches("carma_ctx_destroy", protos["carma_ctx_destroy"], C.c_int, [C.c_void_p])
