"""The kernels of the preparation stream fit in the registers the training step leaves free (CPU only: a device-only compile).

Five waves of k_forward / k_update_fused (96 registers each) leave 32 of a SIMD's 512 registers.  A Localizer or probe wave that
is allocated more than 32 can start only where fewer main-stream waves sit, and keeps a fifth one out while it runs (round 6:
eight registers more in k_loc_emit cost the cold step 15 %, profiles/r06r_*).  The ALLOCATION is what counts: the kernel
descriptor's next free VGPR (AGPRs included) in granules of 8, which the compiler may pad beyond the registers the code uses
(a kernel whose static LDS limits its own occupancy is padded up to what that occupancy allows).
"""
import math
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "difacto_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

BUDGET = 32

# the preparation stream's kernels as the library instantiates them (dfh_pending.hip: launch_loc_stage; dfh_localize_api.hip: the probe), C3's size class
TU = r"""
#include <hip/hip_runtime.h>
#include "dfh_kernels.hip"
#include "dfh_localize.hip"
namespace dfh {
template __global__ void k_loc_count<LOC_MAX_BUCKETS>(LocView);
template __global__ void k_loc_count_gather<LOC_MAX_BUCKETS>(LocView, GatherSrc);
template __global__ void k_loc_scatter<LOC_MAX_BUCKETS>(LocView);
template __global__ void k_loc_emit<false>(LocView, EmitOut, TableView, uint32_t*);
template __global__ void k_loc_emit<true>(LocView, EmitOut, TableView, uint32_t*);
}
"""

KERNELS = {
    "k_loc_count<1024>": "_ZN3dfh11k_loc_countILi1024EEEvNS_7LocViewE",
    "k_loc_count_gather<1024>": "_ZN3dfh18k_loc_count_gatherILi1024EEEvNS_7LocViewENS_9GatherSrcE",
    "k_lookup": "_ZN3dfh8k_lookupENS_9TableView",
    "k_loc_scatter<1024>": "_ZN3dfh13k_loc_scatterILi1024EEEvNS_7LocViewE",
    "k_loc_sort": "_ZN3dfh10k_loc_sortENS_7LocViewE",
    "k_loc_emit<false>": "_ZN3dfh10k_loc_emitILb0EEEvNS_7LocViewENS_7EmitOutENS_9TableViewEPj",
    "k_loc_emit<true>": "_ZN3dfh10k_loc_emitILb1EEEvNS_7LocViewENS_7EmitOutENS_9TableViewEPj",
}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("prep_regs")
    src = d / "prep_kernels.hip"
    src.write_text(TU)
    asm = d / "prep_kernels.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-o", str(asm), str(src)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return asm.read_text(), r.stderr


def _remarks(stderr):
    """kernel-resource-usage remarks: mangled name -> {field: value}"""
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def _descriptors(asm):
    """.amdhsa_kernel blocks: mangled name -> {directive: int}"""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.(amdhsa_\w+) (\d+)", m.group(2))}
    return out


def _find(table, prefix):
    hits = [k for k in table if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    return table[hits[0]]


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_prep_kernel_fits_in_32_registers(compiled, kernel):
    asm, stderr = compiled
    rem = _find(_remarks(stderr), KERNELS[kernel])
    kd = _find(_descriptors(asm), KERNELS[kernel])
    vgpr, agpr = int(rem["VGPRs"]), int(rem["AGPRs"])
    alloc = int(math.ceil(kd["amdhsa_next_free_vgpr"] / 8.0)) * 8   # what the hardware allocates per wave (AGPRs included)
    print("%s: VGPRs %d AGPRs %d next_free_vgpr %d -> %d allocated, scratch %s" % (
        kernel, vgpr, agpr, kd["amdhsa_next_free_vgpr"], alloc, rem["ScratchSize [bytes/lane]"]))
    assert agpr == 0, "%s: AGPRs come out of the same register file" % kernel
    assert int(rem["ScratchSize [bytes/lane]"]) == 0 and kd["amdhsa_private_segment_fixed_size"] == 0, "%s: scratch" % kernel
    assert int(rem["VGPRs Spill"]) == 0, "%s: VGPR spills" % kernel
    assert vgpr <= BUDGET, "%s: %d VGPRs" % (kernel, vgpr)
    assert alloc <= BUDGET, "%s: %d registers allocated per wave (next_free_vgpr %d)" % (kernel, alloc, kd["amdhsa_next_free_vgpr"])
