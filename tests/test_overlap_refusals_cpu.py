"""The refusals of the nine overlap entry points (rtk_dev_triangles_in_box_*, _in_obb_*, _touching_*: one launcher,
rtk_amd/csrc/rtk_overlap_walk.h): the WHOLE text of rtk_amd_last_error() for every call the host can refuse, and which of two
faults a call wrong in two ways is told about. No device is needed: what is refused is refused before the scene is looked at.

EXPECTED holds the texts as the three separate launchers gave them before they became one; <ptr> stands for a pointer printed
with %p."""
import ctypes as C
import re

import pytest

ERR_BAD_ARG = -2

# (C symbol stem, takes the touch filter)
FAMILIES = (("rtk_dev_triangles_in_box", False), ("rtk_dev_triangles_in_obb", False), ("rtk_dev_triangles_touching", True))
FORMS = ("count", "all", "counted")

EXPECTED = {
    "rtk_dev_triangles_in_box_count": {
        "NULL scene": "rtk_dev_triangles_in_box_count: NULL scene",
        "NULL queries": "rtk_dev_triangles_in_box_count: NULL boxes, counts",
        "2^32 queries": "rtk_dev_triangles_in_box_count: 4294967296 queries: a batch holds fewer than 2^32",
        "NULL counts": "rtk_dev_triangles_in_box_count: NULL boxes, counts",
        "list: short struct_size": "rtk_dev_triangles_in_box_count: bad list (struct_size 8, flags 0, d_count <ptr>)",
        "list: flags": "rtk_dev_triangles_in_box_count: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
        "list: no d_count": "rtk_dev_triangles_in_box_count: bad list (struct_size 24, flags 0, d_count (nil))",
        "bad list and 2^32 queries": "rtk_dev_triangles_in_box_count: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
    },
    "rtk_dev_triangles_in_box_all": {
        "NULL scene": "rtk_dev_triangles_in_box_all: NULL scene",
        "NULL queries": "rtk_dev_triangles_in_box_all: NULL boxes, offsets or prims",
        "2^32 queries": "rtk_dev_triangles_in_box_all: 4294967296 queries: a batch holds fewer than 2^32",
        "NULL offsets": "rtk_dev_triangles_in_box_all: NULL boxes, offsets or prims",
        "NULL prims": "rtk_dev_triangles_in_box_all: NULL boxes, offsets or prims",
        "list: short struct_size": "rtk_dev_triangles_in_box_all: bad list (struct_size 8, flags 0, d_count <ptr>)",
        "list: flags": "rtk_dev_triangles_in_box_all: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
        "list: no d_count": "rtk_dev_triangles_in_box_all: bad list (struct_size 24, flags 0, d_count (nil))",
        "bad list and 2^32 queries": "rtk_dev_triangles_in_box_all: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
    },
    "rtk_dev_triangles_in_box_counted": {
        "NULL scene": "rtk_dev_triangles_in_box_counted: NULL scene",
        "NULL queries": "rtk_dev_triangles_in_box_counted: NULL boxes, offsets or prims",
        "2^32 queries": "rtk_dev_triangles_in_box_counted: 4294967296 queries: a batch holds fewer than 2^32",
        "NULL counts": "rtk_dev_triangles_in_box_counted: NULL boxes, counts",
        "NULL prims": "rtk_dev_triangles_in_box_counted: NULL boxes, offsets or prims",
        "NULL counters": "rtk_dev_triangles_in_box_counted: NULL counters",
    },
    "rtk_dev_triangles_in_obb_count": {
        "NULL scene": "rtk_dev_triangles_in_obb_count: NULL scene",
        "NULL queries": "rtk_dev_triangles_in_obb_count: NULL obbs, counts",
        "2^32 queries": "rtk_dev_triangles_in_obb_count: 4294967296 queries: a batch holds fewer than 2^32",
        "NULL counts": "rtk_dev_triangles_in_obb_count: NULL obbs, counts",
        "list: short struct_size": "rtk_dev_triangles_in_obb_count: bad list (struct_size 8, flags 0, d_count <ptr>)",
        "list: flags": "rtk_dev_triangles_in_obb_count: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
        "list: no d_count": "rtk_dev_triangles_in_obb_count: bad list (struct_size 24, flags 0, d_count (nil))",
        "bad list and 2^32 queries": "rtk_dev_triangles_in_obb_count: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
    },
    "rtk_dev_triangles_in_obb_all": {
        "NULL scene": "rtk_dev_triangles_in_obb_all: NULL scene",
        "NULL queries": "rtk_dev_triangles_in_obb_all: NULL obbs, offsets or prims",
        "2^32 queries": "rtk_dev_triangles_in_obb_all: 4294967296 queries: a batch holds fewer than 2^32",
        "NULL offsets": "rtk_dev_triangles_in_obb_all: NULL obbs, offsets or prims",
        "NULL prims": "rtk_dev_triangles_in_obb_all: NULL obbs, offsets or prims",
        "list: short struct_size": "rtk_dev_triangles_in_obb_all: bad list (struct_size 8, flags 0, d_count <ptr>)",
        "list: flags": "rtk_dev_triangles_in_obb_all: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
        "list: no d_count": "rtk_dev_triangles_in_obb_all: bad list (struct_size 24, flags 0, d_count (nil))",
        "bad list and 2^32 queries": "rtk_dev_triangles_in_obb_all: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
    },
    "rtk_dev_triangles_in_obb_counted": {
        "NULL scene": "rtk_dev_triangles_in_obb_counted: NULL scene",
        "NULL queries": "rtk_dev_triangles_in_obb_counted: NULL obbs, offsets or prims",
        "2^32 queries": "rtk_dev_triangles_in_obb_counted: 4294967296 queries: a batch holds fewer than 2^32",
        "NULL counts": "rtk_dev_triangles_in_obb_counted: NULL obbs, counts",
        "NULL prims": "rtk_dev_triangles_in_obb_counted: NULL obbs, offsets or prims",
        "NULL counters": "rtk_dev_triangles_in_obb_counted: NULL counters",
    },
    "rtk_dev_triangles_touching_count": {
        "NULL scene": "rtk_dev_triangles_touching_count: NULL scene",
        "NULL queries": "rtk_dev_triangles_touching_count: NULL triangles, counts",
        "2^32 queries": "rtk_dev_triangles_touching_count: 4294967296 queries: a batch holds fewer than 2^32",
        "NULL counts": "rtk_dev_triangles_touching_count: NULL triangles, counts",
        "list: short struct_size": "rtk_dev_triangles_touching_count: bad list (struct_size 8, flags 0, d_count <ptr>)",
        "list: flags": "rtk_dev_triangles_touching_count: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
        "list: no d_count": "rtk_dev_triangles_touching_count: bad list (struct_size 24, flags 0, d_count (nil))",
        "bad list and 2^32 queries": "rtk_dev_triangles_touching_count: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
        "filter: short struct_size": "rtk_dev_triangles_touching_count: bad filter (struct_size 8, flags 0)",
        "filter: unknown bit": "rtk_dev_triangles_touching_count: bad filter (struct_size 16, flags 0x80000001)",
        "bad filter and 2^32 queries": "rtk_dev_triangles_touching_count: bad filter (struct_size 16, flags 0x2)",
        "bad list and bad filter": "rtk_dev_triangles_touching_count: bad list (struct_size 8, flags 0, d_count <ptr>)",
    },
    "rtk_dev_triangles_touching_all": {
        "NULL scene": "rtk_dev_triangles_touching_all: NULL scene",
        "NULL queries": "rtk_dev_triangles_touching_all: NULL triangles, offsets or prims",
        "2^32 queries": "rtk_dev_triangles_touching_all: 4294967296 queries: a batch holds fewer than 2^32",
        "NULL offsets": "rtk_dev_triangles_touching_all: NULL triangles, offsets or prims",
        "NULL prims": "rtk_dev_triangles_touching_all: NULL triangles, offsets or prims",
        "list: short struct_size": "rtk_dev_triangles_touching_all: bad list (struct_size 8, flags 0, d_count <ptr>)",
        "list: flags": "rtk_dev_triangles_touching_all: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
        "list: no d_count": "rtk_dev_triangles_touching_all: bad list (struct_size 24, flags 0, d_count (nil))",
        "bad list and 2^32 queries": "rtk_dev_triangles_touching_all: bad list (struct_size 24, flags 0x1, d_count <ptr>)",
        "filter: short struct_size": "rtk_dev_triangles_touching_all: bad filter (struct_size 8, flags 0)",
        "filter: unknown bit": "rtk_dev_triangles_touching_all: bad filter (struct_size 16, flags 0x80000001)",
        "bad filter and 2^32 queries": "rtk_dev_triangles_touching_all: bad filter (struct_size 16, flags 0x2)",
        "bad list and bad filter": "rtk_dev_triangles_touching_all: bad list (struct_size 8, flags 0, d_count <ptr>)",
    },
    "rtk_dev_triangles_touching_counted": {
        "NULL scene": "rtk_dev_triangles_touching_counted: NULL scene",
        "NULL queries": "rtk_dev_triangles_touching_counted: NULL triangles, offsets or prims",
        "2^32 queries": "rtk_dev_triangles_touching_counted: 4294967296 queries: a batch holds fewer than 2^32",
        "NULL counts": "rtk_dev_triangles_touching_counted: NULL triangles, counts",
        "NULL prims": "rtk_dev_triangles_touching_counted: NULL triangles, offsets or prims",
        "NULL counters": "rtk_dev_triangles_touching_counted: NULL counters",
        "filter: short struct_size": "rtk_dev_triangles_touching_counted: bad filter (struct_size 8, flags 0)",
        "filter: unknown bit": "rtk_dev_triangles_touching_counted: bad filter (struct_size 16, flags 0x80000001)",
        "bad filter and 2^32 queries": "rtk_dev_triangles_touching_counted: bad filter (struct_size 16, flags 0x2)",
    },
}


def _cases(has_filter, form):
    """name -> keyword arguments of _call that differ from a call that would be let through"""
    cases = {"NULL scene": dict(scene=None), "NULL queries": dict(q=None), "2^32 queries": dict(n=1 << 32)}
    if form == "count":
        cases["NULL counts"] = dict(out=None)
    elif form == "all":
        cases["NULL offsets"] = dict(offsets=None)
        cases["NULL prims"] = dict(prims=None)
    else:
        cases["NULL counts"] = dict(offsets=None, prims=None, out=None)
        cases["NULL prims"] = dict(prims=None)
        cases["NULL counters"] = dict(counters=None)
    if form != "counted":                                            # (the counted forms take no list)
        cases["list: short struct_size"] = dict(lst=dict(struct_size=8))
        cases["list: flags"] = dict(lst=dict(flags=1))
        cases["list: no d_count"] = dict(lst=dict(d_count=None))
        cases["bad list and 2^32 queries"] = dict(lst=dict(flags=1), n=1 << 32)
    if has_filter:
        cases["filter: short struct_size"] = dict(flt=dict(struct_size=8))
        cases["filter: unknown bit"] = dict(flt=dict(flags=0x80000001))
        cases["bad filter and 2^32 queries"] = dict(flt=dict(flags=2), n=1 << 32)
        if form != "counted":
            cases["bad list and bad filter"] = dict(lst=dict(struct_size=8), flt=dict(flags=2))
    return cases


def _call(api, stem, has_filter, form, keep, **kw):
    """One call of stem_form: every argument good (64 bytes of host memory stand for device memory: nothing gets as far as
    reading it) except what kw names. lst / flt: fields of the list / the filter that differ from a good one."""
    dummy = C.cast(keep.setdefault("buf", C.create_string_buffer(64)), C.c_void_p)
    a = dict(scene=dummy, q=dummy, n=4, lst=None, flt=None, out=dummy, offsets=dummy, prims=dummy, counters=C.byref(keep.setdefault("ctr", api.TraceCounters())))
    a.update(kw)
    lst = flt = None
    if a["lst"] is not None:
        l = api.RayList()
        l.struct_size, l.flags, l.d_ids, l.d_count = C.sizeof(api.RayList), 0, None, dummy.value
        for k, v in a["lst"].items():
            setattr(l, k, v)
        lst = C.byref(l)
    if a["flt"] is not None:
        f = api.TouchFilter()
        f.struct_size, f.flags, f.d_first_prim = C.sizeof(api.TouchFilter), 0, None
        for k, v in a["flt"].items():
            setattr(f, k, v)
        flt = C.byref(f)
    filt = (flt,) if has_filter else ()
    fn = getattr(api.lib(), "%s_%s" % (stem, form))
    if form == "count":
        return fn(a["scene"], a["q"], a["n"], lst, *filt, a["out"], None)
    if form == "all":
        return fn(a["scene"], a["q"], a["n"], lst, *filt, a["offsets"], a["prims"], a["out"], None)
    return fn(a["scene"], a["q"], a["n"], *filt, a["offsets"], a["prims"], a["out"], a["counters"])


def _matches(text, expected):
    return re.fullmatch(re.escape(expected).replace(re.escape("<ptr>"), "0x[0-9a-f]+"), text) is not None


def test_every_case_has_its_text():
    for stem, has_filter in FAMILIES:
        for form in FORMS:
            assert set(EXPECTED["%s_%s" % (stem, form)]) == set(_cases(has_filter, form)), (stem, form)
    assert len(EXPECTED) == 9


@pytest.mark.parametrize("stem,has_filter", FAMILIES)
def test_refusal_texts(api, stem, has_filter):
    keep = {}
    for form in FORMS:
        name = "%s_%s" % (stem, form)
        for case, kw in _cases(has_filter, form).items():
            assert _call(api, stem, has_filter, form, keep, **kw) == ERR_BAD_ARG, (name, case)
            assert _matches(api.last_error(), EXPECTED[name][case]), (name, case, api.last_error())
        # and a call with nothing wrong and no queries is let through: the cases above are refused for what they name
        assert _call(api, stem, has_filter, form, keep, n=0) == 0, name
