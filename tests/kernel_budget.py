"""Register, scratch and LDS use of the library's kernels as the shipped build compiles them.

The remarks come from `make resources UNIT=<unit>` in opendht_amd/csrc, i.e. from the compile line
the object rule runs (HIPFLAGS plus the unit's own flags), device code only; hipcc cross-compiles
gfx950, so no GPU is needed.  A unit is compiled once per process.  The caps live in
tests/test_kernel_resources.py."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opendht_amd", "csrc")
# the compiler make will run (`HIPCC ?=`: the environment's, else the Makefile's); None where it is absent
HIPCC = shutil.which(os.environ.get("HIPCC") or
                     re.search(r"^HIPCC \?= (\S+)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1))
MAX_COMPILES = 8          # at once; never sized by the CPU count
_usage = {}


def kernel_units():
    """the Makefile's SRCS without the C ABI's host units (api*.hip)"""
    srcs = re.search(r"^SRCS := (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    return [s[:-len(".hip")] for s in srcs if not s.startswith("api")]


def usage(unit):
    """{mangled kernel name: {"VGPRs": n, "ScratchSize": bytes per lane, "LDS": bytes per block}}"""
    if unit not in _usage:
        out = subprocess.run(["make", "-s", "-C", CSRC, "resources", "UNIT=" + unit],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        kern, res = None, {}
        for line in out.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                kern = m.group(1)
                res[kern] = {}
                continue
            m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and kern:
                res[kern][m.group(1).split()[0]] = int(m.group(2))
        assert res, f"{unit}: no kernel resource remarks parsed"
        _usage[unit] = res
    return _usage[unit]


def compile_all(units):
    """fill the cache for `units`, MAX_COMPILES compiles at a time"""
    with ThreadPoolExecutor(MAX_COMPILES) as ex:
        list(ex.map(usage, units))


def check(unit, caps):
    """The one rule: no kernel of `unit` uses scratch, every kernel matches exactly one fragment of
    `caps` (mangled-name fragment -> max VGPRs), every fragment is seen, VGPRs <= cap."""
    use = usage(unit)
    spills = {k: v["ScratchSize"] for k, v in use.items() if v.get("ScratchSize", 0)}
    assert not spills, f"kernels of {unit}.hip using scratch: {spills}"
    seen = set()
    for k, v in use.items():
        frags = [f for f in caps if re.search(rf"\d{f}", k)]
        assert len(frags) == 1, f"{k}: a kernel of {unit}.hip without a cap" if not frags else f"{k}: matches {frags}"
        seen.add(frags[0])
        assert v["VGPRs"] <= caps[frags[0]], f"{k}: {v['VGPRs']} VGPRs > {caps[frags[0]]}"
    assert seen == set(caps), f"{unit}.hip: kernels not found: {set(caps) - seen}"
