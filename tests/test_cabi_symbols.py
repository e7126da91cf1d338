"""CPU: the C ABI as one contract.  clipself_amd.hip.ABI maps every public header under include/ to its table of ctypes signatures;
for each header the names, the arities, the exports of the built library, the includes and plain C99 are held against the header's text,
the ctypes structs against the C compiler's sizeof / offsetof, and the Python constants against the headers' macros (no compute calls --
there is no GPU in the build container)."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from clipself_amd import hip

ROOT = Path(__file__).resolve().parent.parent
INC = ROOT / "include"
HEADERS = list(hip.ABI)
INCLUDES = {"clipself_hip.h": ["<stddef.h>", "<stdint.h>"]}                    # every other header: <stddef.h> alone
# header -> (HipOps' capability flag, its tensor-level wrappers, the entry points the detector features were merged with)
DETECTOR = {
    "clipself_det.h": ("DET_POST", ["nms", "delta2bbox", "nms_workspace"], ["csd_delta2bbox", "csd_nms", "csd_nms_workspace"]),
    "clipself_roi.h": ("ROI_EXTRACT", ["roi_extract_fwd", "roi_extract_bwd", "roi_extract_workspace"],
                       ["csr_roi_extract_bwd", "csr_roi_extract_fwd", "csr_roi_extract_workspace"]),
    "clipself_assign.h": ("ASSIGN", ["assign", "sample", "bbox_targets", "assign_workspace"], ["csa_assign", "csa_sample", "csa_targets", "csa_workspace"]),
    "clipself_loss.h": ("LOSS", ["rpn_loss", "bbox_head_loss", "loss_workspace"], ["csl_bbox_head_loss", "csl_rpn_loss", "csl_workspace"]),
    "clipself_mask.h": ("MASK", ["mask_target", "mask_loss", "paste_masks", "mask_workspace"],
                        ["csm_mask_loss", "csm_mask_target", "csm_paste_masks", "csm_workspace"]),
    "clipself_rpn.h": ("RPN", ["rpn_select", "rpn_select_workspace"], ["csp_select", "csp_workspace"]),
    "clipself_conv.h": ("CONV3X3", ["conv3x3", "im2col3x3"], ["csc_conv3x3", "csc_im2col3x3"]),
    "clipself_bn.h": ("BATCHNORM", ["bn_stats", "bn_finalize", "bn_apply", "bn_bwd_reduce", "bn_bwd_apply", "bn_workspace"],
                      ["csb_apply", "csb_bwd_apply", "csb_bwd_reduce", "csb_finalize", "csb_row_parts", "csb_stats", "csb_workspace"]),
}


def _text(header):
    return re.sub(r"/\*.*?\*/", "", (INC / header).read_text(), flags=re.S)


def _prefix(header):
    return next(iter(hip.ABI[header])).split("_")[0] + "_"


def _prototypes(header):
    """name -> argument count of every prototype the header declares."""
    found = re.findall(r"\b(" + _prefix(header) + r"[a-z0-9_]+)\s*\(([^)]*)\)", _text(header))
    return {n: len([a for a in args.split(",") if a.strip() not in ("", "void")]) for n, args in found}


def _gcc(tmp_path, name, text, *flags):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / name
    src.write_text(text)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{INC}", str(src), *flags], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def _run_c(tmp_path, name, body):
    """The output lines of a C program that includes all the headers."""
    exe = tmp_path / (name + ".bin")
    _gcc(tmp_path, name + ".c", "".join(f'#include "{h}"\n' for h in HEADERS) + "#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n"
         + body + "    return 0;\n}\n", "-o", str(exe))
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()


def _library():
    if not hip.library_path().exists():
        hip.build_library()
    return hip.load_library()


def test_the_registry_lists_every_public_header():
    assert sorted(HEADERS) == sorted(p.name for p in INC.glob("*.h")) and len(HEADERS) == 9
    assert hip.ABI["clipself_hip.h"] is hip.SIGNATURES and len(hip.SIGNATURES) >= 20


@pytest.mark.parametrize("header", HEADERS)
def test_header_contract(header, tmp_path):
    table, text, prefix = hip.ABI[header], _text(header), _prefix(header)
    protos = _prototypes(header)
    # names: the header's are the table's, and the library exports every one
    assert sorted(protos) == sorted(table), f"hip.ABI[{header!r}] and the header disagree"
    assert all(n.startswith(prefix) for n in table)
    lib = _library()
    for n in table:
        assert hasattr(lib, n), f"{n} declared in include/{header} but not exported"
    # arities: every prototype against its argtypes
    for n, (_, argtypes) in table.items():
        assert protos[n] == len(argtypes), n
    # the prefix belongs to this header alone: no other header declares or mentions it, no other table lists it
    for other in HEADERS:
        if other == header:
            continue
        assert not any(k.startswith(prefix) for k in hip.ABI[other]), (header, other)
        if prefix == "cs_":                                                   # cs_stream_t is every header's; entry points are not
            assert re.findall(r"\bcs_[a-z0-9_]+\s*\(", _text(other)) == [], (header, other)
        else:
            assert prefix not in _text(other), (header, other)
    assert re.findall(r"#\s*include\s*([<\"][^>\"]+[>\"])", text) == INCLUDES.get(header, ["<stddef.h>"])
    # every source file that defines one of these entry points is compiled against this header
    csrc = ROOT / "clipself_amd" / "csrc"
    defined = {}
    for src in list(csrc.glob("*.hip")) + list(csrc.glob("*.cpp")):
        for n in re.findall(r'^extern "C" [^(]*?\b(' + prefix + r'[a-z0-9_]+)\s*\(', src.read_text(), flags=re.M):
            assert f'#include "../../include/{header}"' in src.read_text(), f"{src.name} defines {n} without including {header}"
            defined[n] = src.name
    assert sorted(defined) == sorted(table)
    assert all(Path(src).stem in (csrc / "build.sh").read_text() for src in defined.values())
    # plain C99: alone, after the headers that came before it, and after all the other eight
    _gcc(tmp_path, "alone.c", f'#include "{header}"\nint main(void) {{ cs_stream_t s = 0; return s != 0; }}\n', "-pedantic", "-fsyntax-only")
    before = HEADERS[:HEADERS.index(header)]
    _gcc(tmp_path, "before.c", "".join(f'#include "{h}"\n' for h in before + [header]), "-pedantic", "-fsyntax-only")
    _gcc(tmp_path, "last.c", "".join(f'#include "{h}"\n' for h in HEADERS if h != header) + f'#include "{header}"\n', "-fsyntax-only")
    # the tensor-level face
    if header in DETECTOR:
        flag, wrappers, names = DETECTOR[header]
        assert getattr(hip.HipOps, flag) is True and sorted(table) == names
        for m in wrappers:
            assert callable(getattr(hip.HipOps, m)), m
    if header == "clipself_conv.h":
        from _conv_ref import RefOpsConv
        assert all(callable(getattr(RefOpsConv, n[len(prefix):])) for n in table)


def test_header_is_plain_c_and_links_against_the_library(tmp_path):
    """The headers are the binding contract for non-C++ hosts: a C program that includes all nine and takes the address of every declared
    entry point must link against libclipself_hip.so (no call is made -- there is no GPU here)."""
    _library()
    names = [n for h in HEADERS for n in hip.ABI[h]]
    lib = hip.library_path()
    _gcc(tmp_path, "bind.c", "".join(f'#include "{h}"\n' for h in HEADERS) + "#include <stdio.h>\nint main(void) {\n    const void* table[] = {\n"
         + "".join(f"        (const void*){n},\n" for n in names)
         + '    };\n    printf("%d\\n", (int)(sizeof table / sizeof table[0]));\n    return 0;\n}\n',
         "-o", str(tmp_path / "bind"), f"-L{lib.parent}", "-l:" + lib.name, f"-Wl,-rpath,{lib.parent}", "-Wl,--unresolved-symbols=ignore-in-shared-libs")


def test_ctypes_structs_have_the_c_layout(tmp_path):
    """sizeof and every field's offsetof, as the C compiler sees the headers' structs, equal the ctypes classes'; the field names are the
    header's, in its order."""
    assert sorted(hip.STRUCTS) == sorted(re.findall(r"typedef struct (\w+) \{", "".join(_text(h) for h in HEADERS)))
    body, want = "", []
    for name, cls in hip.STRUCTS.items():
        fields = [f for f, _ in cls._fields_]
        decl = re.search(r"typedef struct " + name + r" \{(.*?)\}", "".join(_text(h) for h in HEADERS), flags=re.S).group(1)
        assert [f.strip().split()[-1].lstrip("*") for f in decl.replace(", ", ";").split(";") if f.strip()] == fields, name
        body += f'    printf("%d\\n", (int)sizeof({name}));\n' + "".join(f'    printf("%d\\n", (int)offsetof({name}, {f}));\n' for f in fields)
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert [int(v) for v in _run_c(tmp_path, "structs", body)] == want


def test_python_constants_are_the_headers_macros(tmp_path):
    """Every limit and layout constant of the headers (CS?_MAX_*, *_EXTRA, CS_ADAMW_GUARD_*) is registered in hip.MACROS, and its value as
    the C compiler evaluates it is the Python constant."""
    in_headers = set(re.findall(r"^#define (CS[A-Z]?_(?:MAX_\w+|\w+_EXTRA|ADAMW_GUARD_\w+))\b", "".join(_text(h) for h in HEADERS), flags=re.M))
    assert in_headers == set(hip.MACROS)
    got = _run_c(tmp_path, "macros", "".join(f'    printf("%lld\\n", (long long)({m}));\n' for m in hip.MACROS))
    assert dict(zip(hip.MACROS, (int(v) for v in got))) == hip.MACROS


def test_ops_refuse_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        hip.HipOps()


def test_every_entry_point_has_a_tensor_level_wrapper_and_a_reference_op():
    """HipOps (product) and RefOps (test infrastructure) both cover the whole C ABI: a wrapper silently dropped from either would
    otherwise only surface on the GPU box."""
    from clipself_amd import hip
    from oracle.ops_ref import RefOps
    renamed = {"cs_crop_resize_u8": "crop_resize", "cs_resize_bilinear_f32": "resize_bilinear"}
    for sym in hip.SIGNATURES:
        if sym in ("cs_last_error", "cs_crop_resize_workspace"):
            continue
        if sym in ("cs_num_compute_units", "cs_stream_create_cu_mask", "cs_stream_destroy"):       # runtime plumbing: nothing to restate
            assert callable(getattr(hip.HipOps, sym[len("cs_"):], None)), f"HipOps.{sym[3:]} missing"
            continue
        name = renamed.get(sym, sym[len("cs_"):])
        assert callable(getattr(hip.HipOps, name, None)), f"HipOps.{name} missing for {sym}"
        assert callable(getattr(RefOps, name, None)), f"RefOps.{name} missing for {sym}"


def test_compute_unit_reservations_compose():
    """HipOps folds three requests into cs_gemm_nt's flags bits 20-27 (compute units a persistent grid leaves free): RCCL's reserve
    (training/distributed.py), the share a prefetched teacher pass leaves to the student, and the cap of the student's own grids.  Teacher side:
    reserve + share; student side: max(reserve, CUs - cap); never fewer than 8 workgroups.  (No GPU: the object is built around the logic.)"""
    from clipself_amd import hip
    ops = hip.HipOps.__new__(hip.HipOps)
    ops.gemm_flags, ops._rccl_reserve, ops._share, ops._cap, ops.num_cus = 0x90, 0, 0, 0, 256
    ops.reserve_compute_units(16)
    assert ops.persistent_grid() == 240 and ops.gemm_flags & 0xFFFFF == 0x90
    ops.share_compute_units(48)                      # the teacher inside the RCCL window of a partitioned run
    assert ops.persistent_grid() == 256 - 64
    ops.reserve_compute_units(0)
    assert ops.persistent_grid() == 208
    ops.share_compute_units(0)
    assert ops.persistent_grid() == 256 and ops.gemm_flags == 0x90
    ops.cap_compute_units(48)                        # the student beside a prefetched pass ...
    assert ops.persistent_grid() == 48
    ops.reserve_compute_units(16)                    # ... with gradient buckets in flight: the cap already leaves RCCL its CUs
    assert ops.persistent_grid() == 48
    ops.cap_compute_units(0)
    assert ops.persistent_grid() == 240
    ops.reserve_compute_units(0)
    with pytest.raises(ValueError):
        ops.cap_compute_units(4)                     # fewer than 8 workgroups: cs_persistent_cap() would ignore it
    ops._cap = 0
    ops.num_cus = 304                                # a 304-CU part (MI300X): the flags field has 8 bits
    ops.cap_compute_units(56)                        # would leave 248 CUs free: encodable
    assert ops.persistent_grid() == 56
    with pytest.raises(ValueError):
        ops.cap_compute_units(48)                    # would leave 256: not encodable -- a ValueError at the call, not an assert inside a step


def test_tower_partition_arguments_are_validated_at_construction(monkeypatch):
    """bad CLIPSELF_PARTITION_* values surface when the method is built (or when the device's CU count is first known), as ValueError."""
    from types import SimpleNamespace
    from clipself_amd.training.clipself import CLIPSelf
    CLIPSelf()                                       # off by default
    CLIPSelf(partition_cus=48)
    for kw in (dict(partition_cus=4), dict(partition_cus=-8), dict(partition_cus=44, partition_mask=True), dict(partition_cus=48, partition_cap=4)):
        with pytest.raises(ValueError):
            CLIPSelf(**kw)
    monkeypatch.setenv("CLIPSELF_PARTITION_CUS", "5")
    with pytest.raises(ValueError):
        CLIPSelf()
    monkeypatch.delenv("CLIPSELF_PARTITION_CUS")
    m = CLIPSelf(partition_cus=48)
    with pytest.raises(ValueError):
        m._check_partition(SimpleNamespace(num_compute_units=lambda: 304))     # the student's cap of 48 would leave 256 CUs free
    m = CLIPSelf(partition_cus=48, partition_cap=64)
    m._check_partition(SimpleNamespace(num_compute_units=lambda: 304))
    assert m._partition_checked


def test_rotary_table_layout_is_checked_by_the_wrapper():
    """Round 6: the layout rope.py:118-142 builds (separable, row part == column part, one entry per rotation pair) is a documented
    precondition of the C ABI.  HipOps verifies it once per table tensor: the oracle's tables and identity tables (the OpenAI-CLIP
    family) pass, also as inference tensors; a table whose row part differs from its column part, whose pair entries differ, or that is not
    separable raises instead of letting a kernel return wrong numbers.  (No GPU: the object is built around the logic.)"""
    import torch
    from clipself_amd import hip
    from oracle.eva_ref import rope_tables
    ops = hip.HipOps.__new__(hip.HipOps)
    cos, sin = rope_tables(14, 64)
    ops._check_rope_tables(cos, sin, 197)
    ops._check_rope_tables(cos, sin, 197)                          # cached
    ops._check_rope_tables(torch.ones(196, 64), torch.zeros(196, 64), 197)
    with torch.inference_mode():
        c2, s2 = cos.clone(), sin.clone()
    ops._check_rope_tables(c2, s2, 197)
    for poke in ((5, 3), (5, 40), (17, 2)):                          # pair partner / column part of one token / row part of one token
        bad = cos.clone()
        bad[poke] += 0.25
        with pytest.raises(ValueError):
            ops._check_rope_tables(bad, sin, 197)
    with pytest.raises(ValueError):
        ops._check_rope_tables(cos[:195], sin[:195], 196)          # not a square grid
    c3, s3 = rope_tables(14, 64)
    c3 = c3.view(14, 14, 64).clone()
    c3[:, :, 32:] = c3[:, :, 32:].flip(1)                          # separable, pairs intact, but column part != row part
    with pytest.raises(ValueError):
        ops._check_rope_tables(c3.view(196, 64), s3, 197)
