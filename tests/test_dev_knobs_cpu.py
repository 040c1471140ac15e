"""Every development knob that csrc reads - a name passed to env_int("AM_...") - is named by something that uses or explains
it: a file under tests/ or tools/, or an .md / .txt file of the repository.  A knob that nothing outside csrc names selects
code that nobody runs: it goes, together with what it selected.  Whole names count (AM_X_Y does not vouch for AM_X)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio-metrics_amd", "csrc")
NAME = re.compile(r"\bAM_[A-Z0-9_]+\b")


def _files(top):
    for folder, dirs, names in os.walk(top):
        dirs[:] = [d for d in dirs if not d.startswith(".") and d != "__pycache__"]
        for name in names:
            yield os.path.join(folder, name)


def _read(path):
    with open(path, errors="ignore") as f:
        return f.read()


def test_every_env_knob_of_csrc_is_named_outside_csrc():
    knobs = {}
    for path in _files(CSRC):
        for name in re.findall(r"\benv_int\(\s*\"(AM_[A-Z0-9_]+)\"", _read(path)):
            knobs.setdefault(name, os.path.relpath(path, ROOT))
    assert len(knobs) >= 20, sorted(knobs)                  # the scan found the knobs at all
    named = set()
    for path in _files(ROOT):
        rel = os.path.relpath(path, ROOT)
        if rel.split(os.sep)[0] in ("tests", "tools") or rel.endswith((".md", ".txt")):
            named.update(NAME.findall(_read(path)))
    orphans = {name: where for name, where in knobs.items() if name not in named}
    assert not orphans, "knobs that no test, tool or document names: %s" % sorted(orphans.items())
