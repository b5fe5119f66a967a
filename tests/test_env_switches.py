"""The environment switches of the C++ library: `getenv(` occurs in csrc/ only inside the three readers (persist_overrides_from_env,
step_overrides_from_env, run_overrides_from_env), so that every host-side decision is a pure function of what they return and can
be pinned without a device (tests/test_persist_choice.py, tests/test_run_plan.py), and every variable they read has a row in
the table of INTEGRATION.md."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READERS = ("persist_overrides_from_env", "step_overrides_from_env", "run_overrides_from_env")


def _reads():
    """{reader: [variable, ...]} over every file of csrc/; a getenv( outside a reader's body raises."""
    out = {r: [] for r in READERS}
    for path in sorted(glob.glob(os.path.join(ROOT, "optical_rl_gym_amd", "csrc", "*"))):
        text = open(path).read()
        bodies = []
        for r in READERS:
            for m in re.finditer(r"static inline \w+ %s\(\) \{" % r, text):
                end = text.index("\n}\n", m.end())
                bodies.append((m.end(), end, r))
        for m in re.finditer(r"\bgetenv\s*\(", text):
            line = text[text.rfind("\n", 0, m.start()) + 1:text.find("\n", m.start())]
            if line.lstrip().startswith("//") and '"' not in line:
                continue  # (prose in a comment)
            owner = [r for a, b, r in bodies if a <= m.start() < b]
            assert owner, "%s: getenv outside the readers: %s" % (os.path.basename(path), line.strip())
            name = re.match(r'\s*\(\s*"([A-Z_0-9]+)"\s*\)', text[m.end() - 1:])
            assert name, "%s: getenv of something that is not a literal name: %s" % (os.path.basename(path), line.strip())
            out[owner[0]].append(name.group(1))
    return out


def test_getenv_only_inside_the_three_readers():
    reads = _reads()
    assert all(reads[r] for r in READERS), reads
    names = [n for r in READERS for n in reads[r]]
    assert len(names) == len(set(names)) == 17 and all(n.startswith("ORL_") for n in names)


def test_every_variable_has_a_row_in_integration_md():
    table = {}
    for line in open(os.path.join(ROOT, "INTEGRATION.md")):
        m = re.match(r"\| `(ORL_[A-Z_0-9]+)` \| `(\w+)` \| (.+?) \| (.+?) \|$", line.strip())
        if m:
            table[m.group(1)] = m.group(2)
    for reader, names in _reads().items():
        for n in names:
            assert table.get(n) == reader, "%s (read by %s) has no row in INTEGRATION.md naming that reader: %s" % (n, reader, table.get(n))
    assert set(table) == {n for names in _reads().values() for n in names}, "a row for a variable the library does not read"
