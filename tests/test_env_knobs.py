"""The environment selects no kernel: a VKZG_* variable read under verkle-kzg_amd/csrc/ is either a
diagnostic (prints only, read in one place) or a test hook that a GPU test names."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "verkle-kzg_amd" / "csrc"
DIAGNOSTIC = {"VKZG_HOST_TIMING", "VKZG_VERBOSE", "VKZG_VERKLE_STAMPS"}
GETENV = re.compile(r'getenv\(\s*"(VKZG_[A-Z0-9_]+)"\s*\)')


def _reads():
    """name -> [(file, line)] of every getenv("VKZG_...") under csrc/"""
    sites = {}
    for path in sorted(CSRC.rglob("*")):
        if path.suffix not in (".hip", ".hpp", ".cpp", ".h"):
            continue
        for no, line in enumerate(path.read_text().splitlines(), 1):
            for name in GETENV.findall(line):
                sites.setdefault(name, []).append((path.relative_to(ROOT).as_posix(), no))
    return sites


def test_every_variable_is_a_diagnostic_or_a_hook_a_gpu_test_names():
    sites = _reads()
    assert sites, "no getenv found: the pattern or the source path is wrong"
    gpu_tests = "\n".join(p.read_text() for p in sorted((ROOT / "tests").glob("test_gpu_*.py")))
    stray = {n: s for n, s in sites.items()
             if n not in DIAGNOSTIC and not re.search(r"\b%s\b" % n, gpu_tests)}
    assert not stray, f"variables no GPU test names: {stray}"


def test_each_diagnostic_variable_is_read_in_one_place():
    sites = _reads()
    for name in sorted(DIAGNOSTIC):
        assert len(sites.get(name, [])) == 1, (name, sites.get(name))
