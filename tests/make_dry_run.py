"""What `make` would run in the package's two build directories, without running it: the command lines that
`make -n` prints (a dry run: nothing is compiled, nothing is written).  The host tests assert on these -- every artefact
links every device library, an object depends on its header -- and not on how a Makefile spells its rules."""
import functools
import os
import subprocess

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcmc-ammsb-gpu_amd")
DEVICE_LIBS = ("hip", "refsample", "readout", "linkpred", "linkcomm", "quality", "cover", "nmi", "omega", "relate")


@functools.lru_cache(maxsize=None)
def commands(subdir, *targets, remake_all=True, touched=()):
    """-> the command lines of `make -n -C mcmc-ammsb-gpu_amd/<subdir> <targets>`, a recipe line that continues over
    several lines as one.  remake_all: as if every target were out of date (-B), so the answer does not depend on what
    is built; otherwise only what is out of date, the files of `touched` (-W) taken as just changed.  What a rule hands
    on to `make` in another directory is part of the answer, as a real run would run it."""
    cmd = ["make", "-n", "--no-print-directory", "-C", os.path.join(PKG, subdir)] + (["-B"] if remake_all else [])
    for path in touched:
        cmd += ["-W", path]
    out = subprocess.run(cmd + list(targets), capture_output=True, text=True, check=True, timeout=300).stdout
    return tuple(ln for ln in out.replace("\\\n", " ").splitlines() if ln.strip())


def host_links():
    """-> the lines of a full host build, sanitizer variants included, that link device libraries (they name
    -lammsb_linkpred); every one of them carries every device library"""
    lines = [ln for ln in commands("host", "all", "asan") if "-lammsb_linkpred" in ln]
    for ln in lines:
        missing = [lib for lib in DEVICE_LIBS if "-lammsb_%s " % lib not in ln + " "]
        assert not missing, (missing, ln)
    return lines


def builds(lines, output, *inputs):
    """does one of the lines write `output` (-o output) from every one of `inputs`?"""
    return any(("-o %s " % output) in ln + " " and all(i in ln for i in inputs) for ln in lines)


def host_all_builds(output, *inputs):
    return builds(commands("host", "all"), output, *inputs)


def csrc_all_builds(output, *inputs):
    return builds(commands("csrc", "all"), output, *inputs)


def hip_library_link():
    """-> the line that links libammsb_hip.so: what it names is what the library is made of"""
    lines = [ln for ln in commands("csrc", "all") if "-o ../libammsb_hip.so " in ln + " "]
    assert len(lines) == 1, lines
    return lines[0]


def header_rebuilds_object(stem):
    """In a built tree: is ammsb_<stem>.o up to date, and compiled again once include/ammsb_<stem>.h has changed?"""
    target, header = "../libammsb_%s.so" % stem, "../../include/ammsb_%s.h" % stem
    obj = "ammsb_%s.o" % stem
    fresh = commands("csrc", target, remake_all=False)
    after = commands("csrc", target, remake_all=False, touched=(header,))
    return not builds(fresh, obj) and builds(after, obj, "-c ammsb_%s.hip" % stem) and builds(after, target, obj)
