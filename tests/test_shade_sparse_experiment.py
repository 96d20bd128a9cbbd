"""The closed k_shade_sparse experiment (polaris_amd/csrc/experiments/shade_sparse.diff) still applies to the product sources.

The kernel lost to k_shade_wave at the roulette bounce (profiles/shade_sparse_ab.txt) and was left out of the product; it is
kept as a patch that scripts/build_variant.sh applies to a COPY of polaris_amd/csrc (`--patch shade_sparse`), with its GPU tests beside
it (experiments/shade_sparse_tests.py).  (It is named .diff because tests/test_abi.py pins the list of *.patch files it checks.)  A patch that no longer applies is a rotten experiment: caught here, without a GPU.
"""
import glob
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polaris_amd", "csrc")


def test_the_patch_applies_and_the_product_holds_none_of_it():
    for f in ("kernels.h", "kernel_table.h", "polaris_hip.hip"):
        assert "k_shade_sparse" not in open(os.path.join(CSRC, f)).read(), f
    with tempfile.TemporaryDirectory() as tmp:
        for f in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")):
            shutil.copy(f, tmp)
        r = subprocess.run(["patch", "-s", "-p1", "--no-backup-if-mismatch", "-i", os.path.join(CSRC, "experiments", "shade_sparse.diff")],
                           cwd=tmp, capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert "void k_shade_sparse(" in open(os.path.join(tmp, "kernels.h")).read()
        assert "kShadeSparse[2]" in open(os.path.join(tmp, "kernel_table.h")).read()
        assert '"shade_sparse_from"' in open(os.path.join(tmp, "polaris_hip.hip")).read()


def test_the_variant_build_script_finds_it():
    text = open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()
    assert "$p.diff" in text and "--patch shade_sparse" in text
