"""tests/alignment_contract.py is total over include/vslam_amd.h: every pointer argument of every entry point (and every
device pointer inside a struct an entry point takes) has exactly one row, and no row names an argument that does not exist.
A new entry point, or a new pointer argument, fails here until its alignment has been decided and written down."""
import ast
import os
import re

import alignment_contract as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# structs that carry device pointers INTO an entry point (vslam_map_arrays / vslam_world_arrays are views handed out)
INPUT_STRUCTS = ("vslam_extract_params", "vslam_pose_outputs")


def header_text():
    text = open(os.path.join(ROOT, "include", "vslam_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _name(decl):
    return re.sub(r"\[.*\]", "", decl.split("*")[-1]).strip().split()[-1]


def header_pointer_args():
    """{entry point: [argument, ...]} for the pointer (and array) arguments of every prototype; a pointer to one of
    INPUT_STRUCTS is followed by `argument->member` for each pointer member of the struct."""
    text = header_text()
    members = {}
    for m in re.finditer(r"typedef struct (\w+) \{(.*?)\} \1;", text, flags=re.S):
        members[m.group(1)] = [_name(part) for decl in m.group(2).split(";") if "*" in decl for part in decl.split(",")]
    out = {}
    for m in re.finditer(r"\b(vslam_[A-Za-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = []
        for decl in (a.strip() for a in m.group(2).split(",")):
            if "*" not in decl and "[" not in decl:
                continue
            args.append(_name(decl))
            t = re.match(r"(?:const\s+)?(\w+)\s*\*", decl)
            if t and t.group(1) in INPUT_STRUCTS:
                args += [f"{args[-1]}->{f}" for f in members[t.group(1)]]
        out[m.group(1)] = args
    return out


def test_parser_sees_the_header():
    args = header_pointer_args()
    assert len(args) >= 100
    assert args["vslam_match_knn2_ratio"] == ["ctx", "d_desc1", "d_n1", "d_desc2", "d_n2", "d_pairs", "d_m", "d_knn"]
    assert args["vslam_view_look_at"] == ["eye", "target", "up", "mv_out"]          # array parameters are pointers
    assert "params->d_pattern" in args["vslam_frontend_pairs"]
    assert "pose->d_points4d" in args["vslam_pipeline_submit_pairs_pose"]
    assert args["vslam_version"] == []


def test_every_pointer_argument_has_exactly_one_row():
    declared = {(e, a) for e, args in header_pointer_args().items() for a in args}
    rows = [(e, a) for e, a, _ in ac.CONTRACT]
    assert len(rows) == len(set(rows)), sorted(r for r in set(rows) if rows.count(r) > 1)
    missing = sorted(declared - set(rows))
    assert not missing, "no row in tests/alignment_contract.py for: " + ", ".join(f"{e}({a})" for e, a in missing)
    stale = sorted(set(rows) - declared)
    assert not stale, "rows for arguments include/vslam_amd.h does not declare: " + ", ".join(f"{e}({a})" for e, a in stale)


def test_no_row_is_written_twice():
    """The table is a dict literal per entry point, where a second row for one argument would silently replace the first."""
    tree = ast.parse(open(ac.__file__.replace(".pyc", ".py")).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.Dict):
            keys = [k.value for k in node.keys if isinstance(k, ast.Constant)]
            assert len(keys) == len(set(keys)), sorted(k for k in set(keys) if keys.count(k) > 1)


def test_requirements_are_well_formed():
    for entry, arg, req in ac.CONTRACT:
        assert req in (ac.HOST, ac.ANY, 4, 8, 16), (entry, arg, req)
        name = arg.split("->")[-1]
        if name.startswith("h_"):
            assert req == ac.HOST, (entry, arg)
        if req != ac.HOST:   # the header's naming convention: device pointers are d_*
            assert name.startswith("d_"), (entry, arg)
    # one requirement per kind of array, wherever it appears
    for kind, want in (("d_desc", 16), ("d_points4d", 16), ("d_matches", 8), ("d_pairs", 8), ("d_xy", 8), ("d_bgr", ac.ANY)):
        got = {req for _, arg, req in ac.CONTRACT if arg.split("->")[-1].startswith(kind)}
        assert got == {want}, (kind, got)


def test_the_header_states_the_contract():
    """The section exists and names every requirement class; each checked entry point's text is the code's business
    (tests/test_gpu_alignment.py), this only keeps the prose from being dropped."""
    raw = open(os.path.join(ROOT, "include", "vslam_amd.h")).read()
    assert "Alignment of device pointers" in raw
    for word in ("16 bytes", "8 bytes", "4 bytes", "any address", "VSLAM_ERR_INVALID"):
        assert word in raw[raw.index("Alignment of device pointers"):][:6000], word
