"""The estimator kernel's emitted gfx950 code (cross-compiled, no GPU needed) keeps the shape docs/ESTIMATOR.md describes: the
window arrives through aligned 16-byte `nt` global loads (the table's pointers did not decay to flat accesses), first[] is
filled with ds_min_u32, every LDS read is an aligned dword read combined with v_alignbyte_b32, the section's counter gets
64-bit global atomics, nothing spills, and the workgroup's LDS is the window plus the table."""
import re

import pytest

from test_isa_invariants import _device_asm


@pytest.fixture(scope="module")
def asm():
    return _device_asm("estimate_kernels")


@pytest.mark.parametrize("lanes", [256, 512, 1024])
def test_estimate_kernel_shape(asm, lanes):
    m = re.search(r"^(_ZN5dxtlt\w*15estimate_kernelILi%dELj32768ELj14EE\w*):\s*(?:;.*)?$" % lanes, asm, re.M)
    assert m, lanes
    body = asm[m.end():]
    body = body[:body.index(".Lfunc_end")]
    lines = [l.strip() for l in body.splitlines() if l.strip() and not l.strip().startswith(";")]
    ops = [l.split()[0] for l in lines]
    assert any(l.startswith("global_load_dwordx4") and l.endswith(" nt") for l in lines)
    assert not any(o.startswith(("flat_", "scratch_", "buffer_")) for o in ops), "a pointer lost its address space, or a spill"
    assert ops.count("ds_min_u32") >= 4                                   # the four grams of a lane's dword pair
    assert "v_alignbyte_b32" in ops
    # LDS reads: whole aligned dwords (single or paired), never a narrower or an unaligned wide one
    assert {o for o in ops if o.startswith("ds_read")} <= {"ds_read_b32", "ds_read2_b32"}
    assert "global_atomic_add_x2" in ops
    assert not any(o.startswith("global_store") for o in ops)             # the counter is the kernel's only output
    desc = asm[asm.index(".amdhsa_kernel " + m.group(1)):]
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1)) == 32768 + 32 + 65536 + 4
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1)) == 0
