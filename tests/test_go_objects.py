"""Static checks of the Go bindings of the objects call and of the get call
(integration/go/objectstore/getobjects_stormck.go, integration/go/storm/get_stormck.go) against
include/stormck.h (CPU, no Go toolchain in the image), in the way of tests/test_go_shim.py: every C.stormck_* call names a
declared function with the declared number of arguments, every C.STORMCK_* constant is defined,
every field of a C struct literal exists in that struct, and the Go mirrors of
stormck_object_result and stormck_get_result have the C field order and sizes."""
import os
import re

from tests.conftest import ROOT
from tests.test_go_shim import HEADER, _balanced, _split_args, _strip_c_comments, header_prototypes

GO_FILES = [os.path.join(ROOT, "integration", "go", "objectstore", "getobjects_stormck.go"),
            os.path.join(ROOT, "integration", "go", "storm", "get_stormck.go")]
CALLS = [{"stormck_objects_host", "stormck_objects_device", "stormck_objects_workspace_bytes", "stormck_last_error"},
         {"stormck_get_host", "stormck_get_device", "stormck_get_workspace_bytes", "stormck_last_error"}]
CONSTS = [{"STORMCK_TRACE_LEAVES_UNVERIFIED", "STORMCK_LOOKUP_NO_SLOT"}, {"STORMCK_TRACE_LEAVES_UNVERIFIED", "STORMCK_LOOKUP_KEY"}]
LITERALS = [{"stormck_scrub_layout", "stormck_pointer", "stormck_blob_params"},
            {"stormck_scrub_layout", "stormck_get_params", "stormck_objectlist_params", "stormck_blob_params"}]


def _read(path):
    with open(path) as f:
        return f.read()


def _code(path):
    """The Go file without its // comments (the cgo preamble is a /* */ comment and stays)."""
    return re.sub(r"//[^\n]*", "", _read(path))


def test_calls_match_header_prototypes():
    protos = header_prototypes()
    for path, must in zip(GO_FILES, CALLS):
        calls = [(m.group(1), len(_split_args(_balanced(_code(path), m.end() - 1))))
                 for m in re.finditer(r"\bC\.(stormck_[a-z_0-9]+)\s*\(", _code(path))]
        assert {name for name, _ in calls} >= must
        for name, nargs in calls:
            assert name in protos, f"{name} is not declared in include/stormck.h"
            assert nargs == protos[name], f"{name}: the binding passes {nargs} args, the header declares {protos[name]}"


def test_constants_are_defined():
    header = _read(HEADER)
    for path, must in zip(GO_FILES, CONSTS):
        consts = set(re.findall(r"\bC\.(STORMCK_[A-Z_0-9]+)", _code(path)))
        assert consts >= must
        for const in consts:
            assert re.search(r"(#define\s+%s\b|\b%s\s*=)" % (const, const), header), const


def _c_struct_fields(name):
    text = _strip_c_comments(_read(HEADER))
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s;" % (name, name), text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.match(r"((?:const\s+)?\w+\s*\*?)\s*(.*)", decl).groups()
        fields += [(n.strip().split("[")[0], ctype.strip()) for n in names.split(",")]
    return fields


def test_struct_literals_name_fields_of_the_c_structs():
    for path, must in zip(GO_FILES, LITERALS):
        text = _code(path)
        literals = list(re.finditer(r"\bC\.(stormck_[a-z_]+)\{", text))
        assert {m.group(1) for m in literals} >= must
        for m in literals:
            body = re.sub(r"C\.stormck_[a-z_]+\{[^{}]*\}", "0", text[m.end():])  # a nested literal is one value
            body = body[:body.index("}")]
            have = {n for n, _ in _c_struct_fields(m.group(1))}
            for field in re.findall(r"(\w+)\s*:", body):
                assert field in have, f"{m.group(1)} has no field {field}"


def test_go_object_result_has_the_c_layout():
    go = re.search(r"type ObjectResult struct \{(.*?)\n\}", _read(GO_FILES[0]), flags=re.S).group(1)
    go_fields = [tuple(line.split()[:2]) for line in go.strip().splitlines()]
    size = {"blocks.ObjectID": 8, "blocks.BlockAddress": 8, "uint64": 8, "uint32": 4, "uint16": 2, "uint8": 1}
    c_size = {"uint64_t": 8, "uint32_t": 4, "uint16_t": 2, "uint8_t": 1}
    c_fields = _c_struct_fields("stormck_object_result")
    assert [size[t] for _, t in go_fields] == [c_size[t] for _, t in c_fields] and sum(size[t] for _, t in go_fields) == 32
    names = [n.lower() for n, _ in go_fields]
    assert names == ["objectid", "address", "reminder", "index", "probes", "status", "_"]
    assert [n.replace("_", "") for n, _ in c_fields][:6] == names[:6] and c_fields[6][0] == "reserved"


def test_go_get_result_has_the_c_layout():
    go = re.search(r"type GetResult struct \{(.*?)\n\}", _read(GO_FILES[1]), flags=re.S).group(1)
    go_fields = [tuple(line.split()[:2]) for line in go.strip().splitlines()]
    size = {"blocks.ObjectID": 8, "blocks.BlockAddress": 8, "uint32": 4, "uint16": 2, "uint8": 1}
    c_size = {"uint64_t": 8, "uint32_t": 4, "uint16_t": 2, "uint8_t": 1}
    c_fields = _c_struct_fields("stormck_get_result")
    assert [size[t] for _, t in go_fields] == [c_size[t] for _, t in c_fields] and sum(size[t] for _, t in go_fields) == 32
    assert [n.lower() for n, _ in go_fields][:6] == [n.replace("_", "") for n, _ in c_fields][:6]


def test_build_tag_and_the_note():
    for path, package in zip(GO_FILES, ("objectstore", "storm")):
        text = _read(path)
        assert text.startswith("//go:build stormck\n") and "Not compiled in this repository" in text
        assert "unsafe.Sizeof(t)" in text and "package " + package in text
