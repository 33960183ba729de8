"""The split weight-gradient kernel lives at one wave per SIMD on all 512 registers (256 accumulators + two plane sets + the reads in flight): a build
that spills puts scratch traffic into the same vector-memory queue as its counted LDS copies and measures nothing.  So the product compile line of
bg_wgrad_split.o and the line of its stamped build (tools/build_stamps.sh bg_wgrad_split) are taken from the Makefile as `make -n` prints them, both
are compiled into a temporary directory with the compiler's resource remarks, and both instantiations (9 and 6 products) of both must come out with
no scratch and at most 256 vector registers."""
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "booster_gym_amd", "csrc")


def test_split_weight_gradient_builds_without_scratch(tmp_path):
    p = subprocess.run(["make", "-n", "-B", "-C", CSRC, f"STAMPS_OBJ={tmp_path}", "bg_wgrad_split.o", f"{tmp_path}/bg_wgrad_split.o"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if "bg_wgrad_split.hip" in l and " -c " in l]
    assert len(lines) == 2 and sum("-DBG_CHAIN_PROBE_STAMPS" in l for l in lines) == 1, p.stdout
    assert all("max-ilp" not in l for l in lines), lines  # both under the default scheduler
    procs = []
    for n, line in enumerate(lines):
        argv = shlex.split(line)
        argv[argv.index("-o") + 1] = str(tmp_path / f"build{n}.o")
        procs.append((line, subprocess.Popen(argv + ["-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for line, proc in procs:
        out = proc.communicate()[0]
        assert proc.returncode == 0, out[-2000:]
        # one block of remarks per kernel of the file; the two instantiations of the split kernel
        blocks = re.findall(r"Function Name: (\S*mlp_wgrad_group_split_kernel\S*)(.*?)(?=Function Name:|\Z)", out, re.S)
        assert len(blocks) == 2, (line, out[-2000:])
        for name, body in blocks:
            scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1))
            vgprs = int(re.search(r"\bVGPRs: (\d+)", body).group(1))
            print(f"{'stamped' if 'PROBE_STAMPS' in line else 'product'} {name}: {vgprs} VGPRs, {scratch} bytes of scratch")
            assert scratch == 0 and vgprs <= 256, (line, name, vgprs, scratch)
