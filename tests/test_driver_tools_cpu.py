"""The command-line driver, tool by tool, against what the driver did before its tools moved into one table.

The driver (metafast_amd/cli/metafast_main.cpp) is built against tests/host/mf_stub.cpp with the stand-alone sanitizer recipe of the other
driver tests: no GPU, every library call fails with a message, so a run shows the driver's own work -- option parsing, the mandatory
arguments, in.properties, the directories made before the first library call, and the whole run for view, bin2fasta and heatmap-maker.
For every tool of `-ts`:
  (a) one run per mandatory argument with that argument left out: exit 1, the message, no in.properties
  (b) a minimal command line with the short option names
  (c) every declared option set away from its default, long names
  further cases for what depends on "given" against "defaulted" (--continue, the two spellings of -b, -b with -bp, the sub-steps)
Exit status, stdout, stderr, the sorted listing of the case's directory and the text of every file the run wrote (in.properties,
out.properties, the sub-steps' too; not the logs) are compared with tests/golden/driver/<tool>.json, the temporary directory normalised
to $TMP and the run's time stamp to $DT.

The goldens were recorded from the driver of the commit BEFORE the table (9019672), never from the code under test:
    g++ <recipe> <that commit's metafast_main.cpp> tests/host/mf_stub.cpp -o old_driver
    python tests/test_driver_tools_cpu.py --record old_driver
"""
import json
import os
import re
import shutil
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "driver")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ENV = dict(os.environ, ASAN_OPTIONS="exitcode=99:detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1:print_stacktrace=1")

# the inputs, written into every case's directory ($TMP): two-record .kmers.bin files, a class file, a 3 x 3 matrix, one component
A, B, C, CLS, MAT, COMP, W = "$TMP/a.kmers.bin", "$TMP/b.kmers.bin", "$TMP/c.kmers.bin", "$TMP/cls.txt", "$TMP/m.txt", "$TMP/comp.bin", "$TMP/w"
INPUTS = {
    "a.kmers.bin": struct.pack(">QhQh", 27, 3, 228, 4), "b.kmers.bin": struct.pack(">QhQh", 27, 5, 99, 1), "c.kmers.bin": struct.pack(">QhQh", 99, 2, 228, 7),
    "cls.txt": b"a\t0\nb\t1\nc\t2\n", "m.txt": b"#\tx\ty\tz\nx\t0\t0.5\t0.25\ny\t0.5\t0\t0.125\nz\t0.25\t0.125\t0\n",
    "comp.bin": struct.pack(">IIqQQ", 1, 2, 2, 27, 228),
}
K = ("k", "-k", ["5"])


def _t(need, more=(), full=(), **extra):
    """need: the mandatory arguments (long name, short token or None, values) in the driver's checking order; more: what (b) adds to them;
    full: what (c) adds, long names; extra: further cases, each one command line or a list of them run one after the other."""
    return dict(need=list(need), more=list(more), full=list(full), extra=extra)


OUT, ST = ["--output-dir", "$TMP/o"], ["--stats-dir", "$TMP/s"]
PV = ["--p-value-chi2", "0.01", "--p-value-mw", "0.02"]
TOOLS = {
    "kmer-counter": _t([K, ("reads", "-i", [A])], full=["--maximal-bad-frequence", "3", *OUT, *ST],
                       cont=[["-k", "5", "-i", A, "-b", "3", "-o", "$TMP/o"], ["-c"], ["-c", "-b", "7"]]),
    "kmer-counter-many": _t([K, ("reads", "-i", [A])], full=["--maximal-bad-frequence", "3", *OUT, *ST]),
    "seq-builder": _t([K, ("k-mers", "-i", [A]), ("sequence-len", "-l", ["7"])], full=["--maximal-bad-frequency", "3", "--bottom-cut-percent", "5", *OUT]),
    "seq-builder-many": _t([K, ("k-mers", "-i", [A]), ("sequence-len", "-l", ["7"])], full=["--maximal-bad-frequency", "3", "--bottom-cut-percent", "5", *OUT],
                           only_b=["-k", "5", "-i", A, "-l", "7", "-b", "3"], only_bp=["-k", "5", "-i", A, "-l", "7", "-bp", "5", "-o", "$TMP/o"]),
    "component-cutter": _t([K, ("sequences", "-i", [A])],
                           full=["--min-seq-len", "50", "--min-component-size", "10", "--max-component-size", "20", "--components-file", "$TMP/o/c.bin"],
                           shorts=["-k", "5", "-i", A, "-l", "9", "-b1", "3", "-b2", "4", "-cm", "$TMP/c2.bin"]),
    "features-calculator": _t([K, ("components-file", "-cm", [COMP])], more=["-ka", A],
                              full=["--reads", B, "--kmers", A, "--selected", C, "--threshold", "2", "--device", "0"], no_input=["-k", "5", "-cm", COMP]),
    "dist-matrix-calculator": _t([("features", None, [MAT, MAT])], full=["--without-names", "--matrix-file", "$TMP/o/x_$DT.txt", "--output-format", "%.2f"]),
    "heatmap-maker": _t([("matrix-file", "-i", [MAT])],
                        full=["--colors-file", CLS, "--without-renumbering", "--newMatrix-file", "$TMP/o/n.txt", "--heatmap-file", "$TMP/h.png", "--invert-colors",
                              "--output-format", "%.2f"],
                        alias=["-i", MAT, "--new-matrix-file", "$TMP/o/n_$DT.txt", "--output-format", "%s", "-wr", "false"]),
    "kmer-counter-posneg": _t([K, ("positiveReads", "-pos", [A]), ("negativeReads", "-neg", [B])], full=["--maximal-bad-frequency", "3", *OUT]),
    "kmers-filter": _t([K, ("k-mers", "-i", [A]), ("filter-kmers", None, [B])], full=["--maximal-bad-frequence", "3", "--max-thresh", "2", *OUT, *ST]),
    "kmers-samples-counter": _t([K, ("k-mers", "-i", [A, B])], full=["--maximal-bad-frequence", "3", *OUT, *ST], no_perc=["-k", "5", "-i", A, "-perc", "3"]),
    "stats-kmers": _t([("a-kmers", "-A", [A]), ("b-kmers", "-B", [B])], full=[*PV, "--maximal-bad-frequence", "2", *OUT],
                      quirk_i=["-A", A, "-B", B, "-i", C, "-b", "4", "-pchi2", "0.5"], bad_p=["-A", A, "-B", B, "-pmw", "x"]),
    "stats-kmers-3": _t([("a-kmers", "-A", [A]), ("b-kmers", "-B", [B]), ("c-kmers", "-C", [C])], full=[*PV, "--maximal-bad-frequence", "2", *OUT],
                        bad_p=["-A", A, "-B", B, "-C", C, "-pchi2", "1.5"]),
    "specific-kmers": _t([("a-kmers", "-A", [A]), ("b-kmers", "-B", [B])], full=[*PV, *OUT], bad_p=["-A", A, "-B", B, "-pchi2", "-1"]),
    "specific-kmers-3": _t([("a-kmers", "-A", [A]), ("b-kmers", "-B", [B]), ("c-kmers", "-C", [C])], full=[*PV, *OUT]),
    "kmers-grouped-counter": _t([K, ("cd-kmers", "-cd", [A]), ("uc-kmers", "-uc", [B]), ("nonibd-kmers", "-nonibd", [C])], more=["-kf", A, B],
                                full=["--kmers-file", A, B, "--maximal-bad-frequence", "3", *OUT, *ST]),
    "kmers-per-sample": _t([K, ("k-mers", "-i", [A, B])], full=["--percent-present", "50", *OUT], perc=["-k", "5", "-i", A, "-perc", "-5"]),
    "unique-kmers": _t([K, ("k-mers", "-i", [A]), ("filter-kmers", None, [B])], full=["--maximal-bad-frequence", "3", *OUT, *ST]),
    "unique-kmers-multi": _t([K, ("k-mers", "-i", [A]), ("filter-kmers", None, [B])],
                             full=["--min-samples", "2", "--max-samples", "3", "--maximal-bad-frequence", "3", *OUT, *ST],
                             min_gt_max=["-k", "5", "-i", A, "--filter-kmers", B, "--min-samples", "3", "--max-samples", "2"]),
    "kmers-multiple-filters": _t([K, ("k-mers", "-i", [A]), ("cd-filter-kmers", "-cd", [A]), ("uc-filter-kmers", "-uc", [B]), ("nonibd-filter-kmers", "-nonibd", [C])],
                                 full=["--maximal-bad-frequence", "3", *OUT, *ST]),
    "kmers-color": _t([K, ("k-mers", "-kf", [A, B]), ("class", None, [CLS])], full=["--maximal-bad-frequency", "3", "--val", *OUT],
                      no_line=["-k", "5", "-kf", MAT, "--class", CLS], val_false=["-k", "5", "-kf", A, "--class", CLS, "-val", "false"]),
    "component-colored": _t([K, ("k-mers", "-i", [A])], full=["--n_groups", "2", "--separate", "--linear", "--n_comps", "4", "--perc", "0.5", *OUT],
                            most=["-k", "5", "-i", A, "-group", "2", "--separate", "--perc", "0.5", *OUT], n_comps=["-k", "5", "-i", A, "-comp", "4"],
                            no_perc=["-k", "5", "-i", A, "-perc", "0.5"]),
    "comp2seq": _t([("components-file", "-cf", [COMP])], full=["--k", "7", "--split"], bad_k=["-cf", COMP, "-k", "32"]),
    "comp2graph": _t([K, ("components-file", "-cf", [COMP])], full=["--k-mers", A, B, "--coverage", "--graph-file", "$TMP/o/g.gfa"], short_i=["-k", "5", "-cm", COMP, "-i", A, "-cov"]),
    "seq2comp": _t([K, ("sequences", "-i", [MAT])], full=["--components-file", "$TMP/o/c.bin"], missing=["-k", "5", "-i", "$TMP/none.fa"]),
    "component-paths": _t([K, ("components-file", "-cf", [COMP]), ("seq", None, [MAT])], more=["-a"],
                          full=["--components", "1", "2", "--all-components", "--min-length", "10", *OUT],
                          shorts=["-k", "5", "-cm", "1", "--components-file", COMP, "--seq", MAT, "-l", "10", "-o", "$TMP/o/p"],
                          none=["-k", "5", "-cf", COMP, "--seq", MAT], bad_no=["-k", "5", "-cf", COMP, "--seq", MAT, "--components", "0"]),
    "view": _t([], more=["-k", "5", "-kf", A], full=["--k", "4", "--kmers-file", A, "--components-file", COMP, "--output-file", "$TMP/o.txt", "--long"],
               nothing=[], comps=["-k", "5", "-cf", COMP], bad_comps=["-k", "5", "-cf", A]),
    "bin2fasta": _t([], more=["-k", "5", "-kf", A, "-o", "$TMP/o/x"], full=["--k", "4", "--kmers-file", A, "--components-file", COMP, "--output-file", "$TMP/p/y", "--split"],
                    stdout=["-k", "5", "-cf", COMP]),
    "matrix-builder": _t([("reads", "-i", [A])],
                         full=["--k", "21", "--maximal-bad-frequency", "2", "--min-seq-len", "50", "--use-reads-for-calculating-features", "--matrix-file", "$TMP/o/m_$DT.txt",
                               "--heatmap-file", "$TMP/o/h_$DT.png", *ST, "--bottom-cut-percent", "5", "--min-component-size", "10", "--max-component-size", "20",
                               "--selected", C, "--without-names", "--output-format", "%.2f", "--colors-file", CLS, "--without-renumbering", "--invert-colors"],
                         other_b=["-i", A, "--maximal-bad-frequence", "4"], both_b=["-i", A, "--maximal-bad-frequence", "4", "-b", "6"], force=["-i", A, "--force"],
                         bad_step=["-i", A, "-s", "no-such-step"], cont=[["-i", A, "-k", "7"], ["-c"]]),
}
# the driver as a whole: listing, help, an unknown tool, the default tool, what is no option
GENERAL = {"ts": ["-ts"], "tools": ["--tools"], "help": ["--help"], "h": ["-h"], "unknown_tool": ["-t", "no-such-tool", "-k", "5"], "default_tool": ["-w", W],
           "unknown_option": ["-t", "kmer-counter", "--no-such-option", "1"], "unknown_short": ["-t", "view", "-zz"], "bare_word": ["-t", "view", "word"],
           "missing_value": ["-t", "kmer-counter", "-k"], "cont_and_force": ["-t", "view", "-c", "--force", "-w", W],
           "launcher_options": ["-ea", "-Xmx4G", "-t", "view", "-w", W, "-v"], "bad_int": ["-t", "kmer-counter", "-k", "x", "-i", A, "-w", W]}


def cases_of(tool):
    """name -> list of command lines (the tool and the work directory are added by run_case)"""
    t = TOOLS[tool]
    flat = lambda need, short: [x for (lng, sht, vals) in need for x in [sht if short and sht else "--" + lng, *vals]]
    cases = {"a_%s" % lng: [flat([n for n in t["need"] if n[0] != lng], True) + t["more"]] for (lng, _, _) in t["need"]}
    cases["b"] = [flat(t["need"], True) + t["more"]]
    cases["c"] = [flat(t["need"], False) + t["full"]]
    for name, cmd in t["extra"].items():
        cases["x_" + name] = cmd if cmd and isinstance(cmd[0], list) else [cmd]
    return cases


STAMP = re.compile(r"\d{4}\.\d\d\.\d\d_\d\d\.\d\d\.\d\d")
DATE = re.compile(r"\d\d-\w{3}-\d{4} \(\w{3}\) \d\d:\d\d:\d\d")


def _norm(s, tmp):
    return DATE.sub("$DATE", STAMP.sub("$DT", s.replace(tmp, "$TMP")))


def run_case(cli, tmp, cmds, tool=None):
    """runs the command lines one after the other in a fresh directory `tmp`; what they did, normalised"""
    os.makedirs(tmp)
    for name, data in INPUTS.items():
        with open(os.path.join(tmp, name), "wb") as f:
            f.write(data)
    runs = []
    for cmd in cmds:
        args = (["-t", tool, "-w", W] if tool else []) + list(cmd)
        r = subprocess.run([cli, *[x.replace("$TMP", tmp) for x in args]], capture_output=True, text=True, errors="replace", env=ENV, timeout=120, input="y\n", cwd=tmp)
        runs.append({"args": args, "exit": r.returncode, "stdout": _norm(r.stdout, tmp), "stderr": _norm(r.stderr, tmp)})
    listing, files = [], {}
    for d, dirs, names in os.walk(tmp):
        rel = os.path.relpath(d, tmp)
        listing += [_norm(os.path.normpath(os.path.join(rel, x)) + "/", tmp) for x in dirs]
        for x in names:
            p = os.path.normpath(os.path.join(rel, x))
            listing.append(_norm(p, tmp))
            if p not in INPUTS and p != os.path.join("w", "log") and not p.startswith(os.path.join("w", "logs")):
                with open(os.path.join(tmp, p), "rb") as f:
                    files[_norm(p, tmp)] = _norm(f.read().decode("utf-8", "replace"), tmp)
    return {"runs": runs, "listing": sorted(listing), "files": files}


def run_tool(cli, base, tool):
    return {name: run_case(cli, os.path.join(base, tool, name), cmds, tool) for name, cmds in cases_of(tool).items()}


def run_general(cli, base):
    return {name: run_case(cli, os.path.join(base, "_general", name), [cmd]) for name, cmd in GENERAL.items()}


def listed_tools(cli, cwd):
    r = subprocess.run([cli, "-ts"], capture_output=True, text=True, env=ENV, timeout=120, cwd=cwd)
    assert r.returncode == 0 and r.stdout.startswith("Available tools:\n"), r.stdout + r.stderr
    return [l.split("\t")[0] for l in r.stdout.splitlines()[1:]]


def _golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def golden_tools():
    return sorted(f[:-5] for f in os.listdir(GOLDEN) if f.endswith(".json") and not f.startswith("_"))


_BUILT = []


def stub_driver():
    """the driver built against the stub, once per process (tests/test_comp2seq_cpu.py asks for it too)"""
    if not _BUILT:
        if not shutil.which("g++"):
            pytest.skip("no g++")
        import atexit
        import tempfile
        d = tempfile.mkdtemp(prefix="metafast_san_")
        atexit.register(shutil.rmtree, d, True)
        out = os.path.join(d, "metafast_san")
        r = subprocess.run(["g++", *SAN, os.path.join(ROOT, "metafast_amd", "cli", "metafast_main.cpp"), os.path.join(ROOT, "tests", "host", "mf_stub.cpp"),
                            "-o", out, "-lpthread"], capture_output=True, text=True)
        if r.returncode != 0 and "sanitize" in r.stderr and "cannot find" in r.stderr:
            pytest.skip("g++ has no sanitizer runtime here")
        assert r.returncode == 0, r.stderr[-3000:]
        _BUILT.append(out)
    return _BUILT[0]


@pytest.fixture(scope="module")
def driver():
    return stub_driver()


def _same(got, want, where):
    assert sorted(got) == sorted(want), (where, sorted(got), sorted(want))
    for name in want:
        g, w = got[name], want[name]
        for i, (gr, wr) in enumerate(zip(g["runs"], w["runs"])):
            for key in ("args", "exit", "stdout", "stderr"):
                assert gr[key] == wr[key], "%s/%s run %d, %s:\n--- now\n%s\n--- before\n%s" % (where, name, i, key, gr[key], wr[key])
        assert len(g["runs"]) == len(w["runs"])
        assert g["listing"] == w["listing"], "%s/%s: the files\n--- now\n%s\n--- before\n%s" % (where, name, "\n".join(g["listing"]), "\n".join(w["listing"]))
        assert sorted(g["files"]) == sorted(w["files"]), (where, name)
        for p in w["files"]:
            assert g["files"][p] == w["files"][p], "%s/%s: %s\n--- now\n%s\n--- before\n%s" % (where, name, p, g["files"][p], w["files"][p])


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_tool_does_what_it_did(driver, tmp_path, tool):
    got, want = run_tool(driver, str(tmp_path), tool), _golden(tool)
    _same(got, want, tool)
    for (lng, sht, _) in TOOLS[tool]["need"]:                          # (a): exit 1, the message, nothing written
        case = got["a_" + lng]
        msg = "ERROR: Mandatory argument --%s%s not set\n" % (lng, " (%s)" % sht if sht else "")
        assert case["runs"][0]["exit"] == 1 and case["runs"][0]["stderr"] == msg, case["runs"][0]
        assert "w/in.properties" not in case["listing"], case["listing"]
    assert "w/in.properties" in got["b"]["listing"] and "w/in.properties" in got["c"]["listing"]


def test_the_driver_as_a_whole(driver, tmp_path):
    _same(run_general(driver, str(tmp_path)), _golden("_general"), "_general")


def test_listed_known_and_tested_tools_are_the_same_set(driver, tmp_path):
    listed = listed_tools(driver, str(tmp_path))
    assert len(set(listed)) == len(listed)
    assert set(listed) == set(golden_tools()) == set(TOOLS)
    for i, tool in enumerate(sorted(set(listed) | set(TOOLS)) + ["no-such-tool", "kmer-counter-", "Kmer-counter"]):
        r = subprocess.run([driver, "-t", tool, "-w", str(tmp_path / ("w%d" % i))], capture_output=True, text=True, env=ENV, timeout=120, input="y\n", cwd=str(tmp_path))
        assert (r.stderr == "ERROR: Tool '%s' not found !\n" % tool and r.returncode == 1) == (tool not in listed), (tool, r.stderr)


def test_every_tool_has_its_cases():
    for tool in golden_tools():
        g = _golden(tool)
        n_a = sum(1 for c in g if c.startswith("a_"))
        assert n_a == len(TOOLS[tool]["need"]) and "b" in g and (n_a > 0 or "c" in g), tool
        assert not any(tok.startswith("--") for tok in g["b"]["runs"][0]["args"] if tok not in ("--features", "--filter-kmers", "--class", "--seq")), tool
        assert not any(re.match(r"-[A-Za-z]", tok) for tok in g["c"]["runs"][0]["args"][4:]), tool


# The defaults of case (b) that a run shows without the GPU: the directories a tool makes before its first library call.  (tool, the
# parameter in in.properties): the list is what the driver of the parent commit does -- kmer-counter, say, calls the library first.
MADE_BEFORE_THE_LIBRARY = [
    ("kmer-counter-many", "sub-counter"), ("kmers-filter", "output-dir"), ("kmers-samples-counter", "output-dir"), ("kmers-samples-counter", "stats-dir"),
    ("stats-kmers", "output-dir"), ("stats-kmers-3", "output-dir"), ("specific-kmers", "output-dir"), ("specific-kmers-3", "output-dir"),
    ("kmers-grouped-counter", "output-dir"), ("kmers-grouped-counter", "stats-dir"), ("kmers-per-sample", "output-dir"), ("kmers-color", "output-dir"),
    ("component-colored", "output-dir"), ("features-calculator", "vectors"), ("kmer-counter-posneg", "pos"),
    ("matrix-builder", "kmer-counter-many"),
]


def test_the_defaults_in_in_properties_are_what_the_run_used(driver, tmp_path):
    for tool, param in MADE_BEFORE_THE_LIBRARY:
        tmp = str(tmp_path / tool / param)
        got = run_case(driver, tmp, cases_of(tool)["b"], tool)
        props = dict(l.split(" = ", 1) for l in got["files"]["w/in.properties"].splitlines())
        if param in props:                                             # a declared parameter: its default is the directory that now exists
            assert props[param].startswith("$TMP/w/"), (tool, param, props)
            made = props[param][len("$TMP/"):] + "/"
        else:                                                          # a fixed name under the work directory
            made = os.path.normpath("w/" + param) + "/"
        assert made in got["listing"] and made in _golden(tool)["b"]["listing"], (tool, param, got["listing"])
    # the tools that finish: heatmap-maker's default --output-format is the one its matrix is printed in, view's and bin2fasta's -k the k-mers' length
    hm = run_case(driver, str(tmp_path / "hm"), cases_of("heatmap-maker")["b"], "heatmap-maker")
    assert "output-format = %.4f\n" in hm["files"]["w/in.properties"] and "\t0.5000\t" in hm["files"]["m_renumbered.txt"], hm["files"]
    mb = run_case(driver, str(tmp_path / "mb"), cases_of("matrix-builder")["b"], "matrix-builder")
    sub = mb["files"]["w/kmer-counter-many/in.properties"]
    assert "k = 31\n" in mb["files"]["w/in.properties"] and "k = 31\n" in sub and "maximal-bad-frequence = 1\n" in sub, sub
    assert "stats-dir = $TMP/w/kmer-counter-many/stats\n" in mb["files"]["w/in.properties"] and "stats-dir = $TMP/w/kmer-counter-many/stats\n" in sub


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: test_driver_tools_cpu.py --record <driver built from the commit before the change, against tests/host/mf_stub.cpp>")
    import tempfile
    cli = os.path.abspath(sys.argv[2])
    os.makedirs(GOLDEN, exist_ok=True)
    with tempfile.TemporaryDirectory() as base:
        listed = listed_tools(cli, base)
        assert set(listed) == set(TOOLS), sorted(set(listed) ^ set(TOOLS))
        for name, res in [(t, run_tool(cli, base, t)) for t in listed] + [("_general", run_general(cli, base))]:
            with open(os.path.join(GOLDEN, name + ".json"), "w") as f:
                json.dump(res, f, indent=1, sort_keys=True)
                f.write("\n")
    print("recorded %d tools" % len(listed))
