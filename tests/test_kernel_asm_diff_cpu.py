"""tools/kernel_asm_diff.py on literal assembly: what its normaliser drops (comments, spacing, the
per-file index of local labels) and what its chunker keeps apart per symbol (body, kernel descriptor,
resource lines, metadata record), so that a kernel moved to another file compares equal and a changed
instruction or register count does not.  No compile."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "kernel_asm_diff", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                    "kernel_asm_diff.py"))
kad = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kad)

K = "_ZN12_GLOBAL__N_11kEPf"


def asm(idx, pad="", insn="v_add_f32_e32 v0, v0, v1", vgpr=4, cuid="aa"):
    """One kernel K as the idx-th function of a file, comments padded by pad."""
    return f"""\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.file\t"x{idx}.hip"
\t.globl\t{K} ; -- Begin function {K}
{K}:{pad}  ; @{K}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[0:1], 0x0
\ts_cbranch_scc1 .LBB{idx}_2
.LBB{idx}_1:{pad}                                ;   in Loop: Header=BB{idx}_1 Depth=1
\t{insn}
\ts_cbranch_vccnz .LBB{idx}_1
.LBB{idx}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {K}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{idx}:
\t.size\t{K}, .Lfunc_end{idx}-{K}
{pad}                                        ; -- End function
\t.set {K}.num_vgpr, {vgpr}
\t.set {K}.private_seg_size, 0
; NumVgprs: {vgpr}
\t.type\t__hip_cuid_{cuid},@object
__hip_cuid_{cuid}:
\t.byte\t0
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
    .name:           {K}
    .vgpr_count:     {vgpr}
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
...
\t.end_amdgpu_metadata
"""


def test_normalise_drops_comments_spacing_and_label_index():
    assert kad.normalise(".LBB3_2:        ;   in Loop: Header=BB3_1 Depth=1") == ".LBB#_2:"
    assert kad.normalise("\ts_cbranch_scc1   .LBB17_2") == kad.normalise("  s_cbranch_scc1 .LBB3_2 ; taken")
    assert kad.normalise("\t.long\t.LJTI4_0-.LBB4_7") == ".long .LJTI#_0-.LBB#_7"
    assert kad.normalise("; NumVgprs: 21") == "" and kad.normalise('\t.file\t"a.hip"') == ""
    assert kad.normalise("\tv_add_f32_e32 v0, v0, v1") != kad.normalise("\tv_add_f32_e32 v0, v0, v2")


def test_chunks_are_cut_per_symbol():
    c = kad.chunks(asm(3))
    assert set(c) == {kad.REST, K, K + " (kernel descriptor)", K + " (resources)", K + " (metadata)"}
    assert c[K][0] == K + ":" and "s_endpgm" in c[K] and not any(l.startswith(".amdhsa") for l in c[K])
    assert not any(l.startswith(".Lfunc_end") for l in c[K])  # the body ends there
    assert c[K + " (kernel descriptor)"][0] == ".amdhsa_kernel " + K
    assert c[K + " (kernel descriptor)"][-1] == ".end_amdhsa_kernel"
    assert c[K + " (resources)"] == [f".set {K}.num_vgpr, 4", f".set {K}.private_seg_size, 0"]
    assert c[K + " (metadata)"] == ["- .agpr_count: 0", ".args:", "- .offset: 0", ".size: 8", f".name: {K}",
                                    ".vgpr_count: 4"]
    assert not any("__hip_cuid_" in l for l in c[kad.REST])
    assert "amdhsa.target: amdgcn-amd-amdhsa--gfx950" in c[kad.REST]


def test_moved_kernel_compares_equal():
    a, b = kad.chunks(asm(3)), kad.chunks(asm(17, pad="      ", cuid="bb"))
    assert kad.differing(a, b) == []
    lines, bad = kad.tree_report({"old.hip": a}, {"new.hip": b}, "rev")
    assert bad == 0 and "files only in rev: 1 kernel descriptors; files only in the working tree: 1" in lines


def test_changed_instruction_and_register_count_compare_unequal():
    a = kad.chunks(asm(3))
    assert kad.differing(a, kad.chunks(asm(3, insn="v_sub_f32_e32 v0, v0, v1"))) == [K]
    d = kad.differing(a, kad.chunks(asm(3, vgpr=5)))
    assert d == sorted([K + " (kernel descriptor)", K + " (resources)", K + " (metadata)"])
    lines, bad = kad.tree_report({"old.hip": a}, {"new.hip": kad.chunks(asm(9, vgpr=5))}, "rev")
    assert bad == 3 and f"differs: {K} (kernel descriptor) (old.hip -> new.hip)" in lines


def test_tree_report_names_missing_and_duplicated_symbols():
    a = kad.chunks(asm(0))
    lines, bad = kad.tree_report({"old.hip": a}, {"one.hip": a, "two.hip": a}, "rev")
    assert bad == 4 and f"defined in 2 files of the working tree: {K} (one.hip, two.hip)" in lines
    lines, bad = kad.tree_report({"old.hip": a}, {"new.hip": {kad.REST: a[kad.REST]}}, "rev")
    assert bad == 4 and f"only in rev: {K} (old.hip)" in lines
