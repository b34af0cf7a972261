"""The A/B switches, from source and docs only: the native library reads its environment in one place (vpd_amd/csrc/switches.h, one
table of field, variable, default), and SWITCHES.md lists exactly the switches that the library and the Python layer read."""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "vpd_amd", "csrc", "switches.h")
NATIVE_SOURCES = (".h", ".hpp", ".hip", ".cpp", ".cc", ".c")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def table():
    """[(field, environment name, default)] of the VPD_SWITCHES list"""
    src = _read(TABLE)
    body = src[src.index("#define VPD_SWITCHES(X)"):src.index("struct VpdSwitches")]
    rows = re.findall(r'X\(\s*(\w+)\s*,\s*"(\w+)"\s*,\s*(-?\d+)\s*\)', body)
    assert len(rows) == body.count("X("), "a row of the table does not parse"
    return [(f, e, int(d)) for f, e, d in rows]


def python_reads():
    """VPD_* names the Python layer reads through os.environ"""
    files = glob.glob(os.path.join(REPO, "vpd_amd", "**", "*.py"), recursive=True)
    files += [os.path.join(REPO, f) for f in ("train_vpd_model.py", "apply_vpd_model.py", "bench.py")]
    names = set()
    for path in files:
        for line in _read(path).splitlines():
            if re.search(r"\bos\.(environ|getenv)\b", line):
                names.update(re.findall(r"""["'](VPD_\w+)["']""", line))
    return names


def documented():
    """switch names SWITCHES.md lists (-DVPD_... build flags are not switches)"""
    return set(re.findall(r"(?<!-D)\bVPD_\w+", _read(os.path.join(REPO, "SWITCHES.md"))))


def test_the_table_is_the_only_environment_reader_of_the_native_code():
    hits = []
    for root in (os.path.join(REPO, "vpd_amd", "csrc"), os.path.join(REPO, "include")):
        for d, _, files in os.walk(root):
            for f in files:
                if f.endswith(NATIVE_SOURCES):
                    path = os.path.join(d, f)
                    hits += [(path, line) for line in _read(path).splitlines() if "getenv" in line]
    assert len(hits) == 1, hits
    path, line = hits[0]
    assert path == TABLE and line.lstrip().startswith("#define VPD_SWITCH_READ"), hits
    src = _read(TABLE)
    assert src.index("inline const VpdSwitches& vpd_switches()") < src.index(line) < src.index("return s;")


def test_table_names_are_unique_and_every_field_is_used():
    rows = table()
    assert len(rows) >= 40
    fields = [f for f, _, _ in rows]
    envs = [e for _, e, _ in rows]
    assert len(set(fields)) == len(fields), fields
    assert len(set(envs)) == len(envs), envs
    assert all(e.startswith("VPD_") for e in envs), envs
    native = "".join(_read(p) for p in glob.glob(os.path.join(REPO, "vpd_amd", "csrc", "*")) if p.endswith(NATIVE_SOURCES))
    unused = [f for f in fields if not re.search(r"vpd_switches\(\)\s*\.\s*%s\b" % f, native)]
    assert not unused, unused


def test_switches_md_lists_every_switch_the_library_reads():
    missing = [e for _, e, _ in table() if e not in documented()]
    assert not missing, missing


def test_switches_md_lists_every_switch_python_reads():
    py = python_reads()
    assert {"VPD_LIB_PATH", "VPD_DDP_OVERLAP", "VPD_LAZY_GRADS"} <= py, py
    missing = sorted(py - documented())
    assert not missing, missing


def test_every_switch_in_switches_md_is_read():
    read = {e for _, e, _ in table()} | python_reads()
    stale = sorted(documented() - read)
    assert not stale, stale
