"""Build libvf_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

    python -m variantformer_amd.csrc.build [--force]

The shared object is written next to the sources (in-tree, git-ignored) so that it travels to the
GPU box with the repo snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ["vf_gemm.hip", "vf_attn.hip", "vf_misc.hip", "vf_forest.hip", "vf_topk.hip", "vf_neighbors.hip", "vf_linkage.hip", "vf_umap.hip", "vf_spectral.hip", "vf_umap_transform.hip", "vf_components.hip", "vf_tsne.hip", "vf_enrich.hip", "vf_kmeans.hip", "vf_silhouette.hip", "vf_bpe.cpp", "vf_vcf.cpp", "vf_host.cpp"]
INCLUDE = os.path.join("..", "..", "include")
HEADERS = ["vf_common.h"] + [os.path.join(INCLUDE, h) for h in sorted(os.listdir(os.path.join(HERE, INCLUDE))) if h.endswith(".h")]
LIB = os.path.join(HERE, "libvf_hip.so")
ARCH = "gfx950"
# vf_attn: scores are never NaN by construction (finite inputs, -inf only as a mask), so fmaxf needs no
# canonicalising v_max in front of every max (68 extra VALU instructions per key tile otherwise).
# The NaN CONTRACTS of this file's kernels (vf_attn_probs: a NaN in a K row / query row makes that head's / that
# row's probabilities NaN) therefore rest on what this compiler emits, not on what the flag guarantees: no kernel here tests for
# NaN, a NaN operand travels through the MFMAs, v_exp, the sums and the final multiply in hardware, and v_max_f32 returns its
# non-NaN operand.  Formally the flag lets a compiler assume the NaN away; tests/test_nonfinite_gpu.py and
# tests/test_attn_probs_gpu.py hold every entry to the contract on the built library, so a compiler that uses the licence fails
# them instead of shipping.
EXTRA_FLAGS = {"vf_attn.hip": ["-fno-honor-nans"]}
# No packed-fp32 VALU instructions (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) in any device code.  Measured on MI355X in
# round 6 (scripts/probes/pk_hazard_probe.hip, profiles/r06_d_pk_hazard_probe.log): a packed-fp32 instruction whose op_sel
# takes the HIGH dword of src1 for the low result (op_sel:[0,1,..] -- what hipcc's SLP vectoriser emits for `vec * scalar`,
# e.g. the LayerNorm-consumer epilogue acc * rstd + t) computes with a wrong src1 in lanes 48..63 while a wave of ANOTHER
# kernel on the same SIMD issues MFMAs (up to 0.6 % of the results beside dense v_mfma_f32_16x16x32_bf16; never alone, never
# beside anything else, never for the other op_sel / op_sel_hi forms or for scalar v_fma_f32).  In one stream kernels do not
# overlap, so the default path never met it; two streams did (the CRE side-stream experiment's 7e-4 run-to-run differences,
# LayerNorm-consumer GEMMs beside the cross attention: scripts/probes/concurrency_probe4.py).  The compiler chooses the op_sel
# form, so the instructions are switched off as a whole: results are bit-identical (a v_pk_fma_f32 is two v_fma_f32), the GEMM
# epilogues cost +0.9 % GEMM time (profiles/r06_d_nopk_cost.txt).  tests/test_build_flags.py keeps the library free of them.
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(HERE, f)) > t for f in SOURCES + HEADERS + [os.path.basename(__file__)])   # flags live here


def build_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale():
        return LIB
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libvf_hip.so")
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(HERE, os.path.splitext(src)[0] + ".o")
        cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result",
               "-mllvm", "-amdgpu-mfma-vgpr-form=1"] + (NO_PACKED_FP32 if src.endswith(".hip") else []) + \
              EXTRA_FLAGS.get(src, []) + \
              ["-c", os.path.join(HERE, src), "-o", obj]
        if verbose:
            cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out}")
        if verbose and out:
            print(out)
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB + ".tmp"] + objs + ["-lz"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}")
    os.replace(LIB + ".tmp", LIB)
    return LIB


if __name__ == "__main__":
    print(build_lib(force="--force" in sys.argv, verbose="-v" in sys.argv))
