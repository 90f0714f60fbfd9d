"""k_fixed_lds stages a workgroup in ONE memory round trip: the gfx950 ISA of
every instantiation, checked without a GPU.

qb_quorum.hip is compiled to assembly with the Makefile's own `asm` command
line (skipped when hipcc is absent) and each k_fixed_lds<N, GPT, VOTE> body is
read as text:

  * between its first and last global_load_lds there is no s_waitcnt with a
    vmcnt field (a wait there leaves the later DMA pieces to a second round
    trip of their own);
  * exactly one such wait precedes the first ds_read of the landing buffer,
    it is a vmcnt(0) and it follows the last DMA;
  * the 2-byte mask loads are all issued before that wait.

The workgroup barrier after the wait was measured and kept,
so its absence is not asserted; neither is `nt` on the mask loads, which
measured slower.

On the commit before this file, <5,4,true> fails the first two: the compiler
hoisted a mask unpack above the tenth DMA, waited there, issued the tenth DMA
and waited again.
"""
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "etcd_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

_KERNEL = re.compile(r"^(_ZN2qb11k_fixed_ldsILi(\d+)ELi(\d+)ELb([01])E\w*):")


def _asm_command(out_dir):
    """The Makefile's own command line for qb_quorum.s (from `make -n asm`),
    with its build directory pointed at ``out_dir``."""
    plan = subprocess.run(["make", "-n", "-C", CSRC, "asm", "HIPCC=" + HIPCC, "BUILD=" + out_dir],
                          check=True, capture_output=True, text=True).stdout
    lines = [ln for ln in plan.splitlines() if "qb_quorum.hip" in ln and " -S " in ln]
    assert len(lines) == 1, plan
    return shlex.split(lines[0])


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(N, GPT, VOTE): [instruction lines]} of every k_fixed_lds instantiation."""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa"))
    subprocess.run(_asm_command(out), check=True, cwd=CSRC, capture_output=True, text=True)
    found, cur = {}, None
    with open(os.path.join(out, "qb_quorum.s")) as f:
        for line in f:
            m = _KERNEL.match(line)
            if m:
                cur = found.setdefault((int(m.group(2)), int(m.group(3)), m.group(4) == "1"), [])
                continue
            if cur is None:
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            ins = line.split(";", 1)[0].strip()
            if ins and not ins.startswith(".") and not ins.endswith(":"):
                cur.append(ins)
    return found


def _is_vm_wait(ins):
    return ins.startswith("s_waitcnt") and "vmcnt" in ins


def _where(body, pred):
    return [i for i, ins in enumerate(body) if pred(ins)]


def test_every_instantiation_present(kernels):
    want = {(n, 4 if n <= 5 else 2, v) for n in range(1, 9) for v in (False, True)}
    assert set(kernels) == want


@pytest.mark.parametrize("vote", [True, False], ids=["vote", "commit"])
@pytest.mark.parametrize("n", range(1, 9))
def test_one_round_trip(kernels, n, vote):
    gpt = 4 if n <= 5 else 2
    body = kernels[(n, gpt, vote)]
    dma = _where(body, lambda s: s.startswith("global_load_lds"))
    reads = _where(body, lambda s: s.startswith("ds_read"))
    waits = _where(body, _is_vm_wait)
    assert len(dma) == n * gpt // 2, "one dwordx4 piece per row and 2 groups of a lane"
    assert all(body[i].startswith("global_load_lds_dwordx4") and body[i].endswith(" nt")
               for i in dma)
    assert reads and reads[0] > dma[-1]
    split = [body[i] for i in waits if dma[0] < i < dma[-1]]
    assert not split, f"wait between the DMA pieces: {split}"
    before = [body[i] for i in waits if i < reads[0]]
    assert len(before) == 1, f"waits before the first ds_read: {before}"
    assert "vmcnt(0)" in before[0]
    the_wait = [i for i in waits if i < reads[0]][0]
    assert the_wait > dma[-1]
    masks = _where(body, lambda s: s.startswith("global_load_ushort"))
    assert len(masks) == (gpt if vote else 0), "voted + granted pair per piece"
    for i in masks:
        assert i < the_wait, "mask load after the wait: a second round trip"
