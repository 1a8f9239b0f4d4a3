"""The command lines of the five K-population tools (dxy / fst / pi / dstat / f3 WindowPops) that end BEFORE a file is opened or
the device is touched, whose exit code, stdout and stderr tests/golden/pops_cli_texts.json pins byte for byte.  One list, issued
twice: by tests/golden/make_pops_cli_texts.py on the commit the fixture is recorded from, and by tests/test_cli_pops_texts_cpu.py
on the tree under test.

Every case is (key, tool, arguments).  The MAF paths are names that do not exist: a case that got as far as opening one would say
`Unable to open` (and start the device beside it), so no case here may be a command line the tool accepts."""
import subprocess

# tool -> (fewest, most MAF files)
TOOLS = {"dxyWindowPops": (2, 8), "fstWindowPops": (2, 8), "piWindowPops": (1, 8), "dstatWindowPops": (4, 7), "f3WindowPops": (3, 6)}
JACKKNIFE = ("dstatWindowPops", "f3WindowPops")
WINDOWS = ["-fixedsite", "1", "-winsize", "2", "-stepsize", "1"]
OUT = ["-out", "o"]


def mafs(k):
    return [f"no_such_pop{i + 1}.mafs" for i in range(k)]


def cases():
    out = []
    for tool, (lo, hi) in TOOLS.items():
        ok = mafs(lo)

        def add(what, args, tool=tool):
            out.append((f"{tool}: {what}", tool, args))

        add("no arguments", [])
        add("option without its value", WINDOWS + OUT + ["-minind"])
        add("unknown option", ["-bogus", "1"] + WINDOWS + OUT + ok)
        add("no -out", WINDOWS + ok)
        add("empty -out", WINDOWS + ["-out", ""] + ok)
        add("one file too few", WINDOWS + OUT + mafs(lo - 1))
        add("one file too many", WINDOWS + OUT + mafs(hi + 1))
        add("-fixedsite 0 without -sizefile", ["-fixedsite", "0", "-winsize", "2", "-stepsize", "1"] + OUT + ok)
        add("-minind 0", ["-minind", "0"] + WINDOWS + OUT + ok)
        add("-winsize without -stepsize", ["-fixedsite", "1", "-winsize", "2"] + OUT + ok)
        add("-stepsize above -winsize", ["-fixedsite", "1", "-winsize", "2", "-stepsize", "3"] + OUT + ok)
        add("-winsize 0 without -fixedsite 1", ["-winsize", "0", "-sizefile", "no_such_sizes.tsv"] + OUT + ok)
        # the order of the refusals: the file count before -out, -out before the options' own checks
        add("too few files and no -out", WINDOWS + mafs(lo - 1))
        add("no -out and no size file", ["-winsize", "2", "-stepsize", "1"] + ok)
        if tool in JACKKNIFE:
            add("-jackknife 2", WINDOWS + ["-jackknife", "2"] + OUT + ok)
            add("-jackknife 1 -winsize 0", ["-fixedsite", "1", "-winsize", "0", "-jackknife", "1"] + OUT + ok)
            add("-jackknife 1 without -winsize", ["-fixedsite", "1", "-jackknife", "1"] + OUT + ok)
            add("-jackknife 1 -winsize 100 -stepsize 50", ["-fixedsite", "1", "-winsize", "100", "-stepsize", "50", "-jackknife", "1"] + OUT + ok)
            add("-jackknife 1 before a later -winsize 0", ["-fixedsite", "1", "-winsize", "100", "-stepsize", "100", "-jackknife", "1", "-winsize", "0"] + OUT + ok)
            add("-jackknife 1 before its -winsize and a -stepsize below it", ["-fixedsite", "1", "-jackknife", "1", "-winsize", "100", "-stepsize", "50"] + OUT + ok)
            # an own option is refused while the options are read: before the file count
            add("-jackknife 2 and too few files", WINDOWS + ["-jackknife", "2"] + OUT + mafs(lo - 1))
        else:
            add("-jackknife 1 given to a tool without it", WINDOWS + ["-jackknife", "1"] + OUT + ok)
        if tool == "dstatWindowPops":
            add("-fd 2", WINDOWS + ["-fd", "2"] + OUT + ok)
            add("-fd 2 and no -out", WINDOWS + ["-fd", "2"] + ok)
        else:
            add("-fd 1 given to a tool without it", WINDOWS + ["-fd", "1"] + OUT + ok)
        if tool == "fstWindowPops":
            add("-estimator x", WINDOWS + ["-estimator", "x"] + OUT + ok)
            add("-estimator x and too many files", WINDOWS + ["-estimator", "x"] + OUT + mafs(hi + 1))
        else:
            add("-estimator wc given to a tool without it", WINDOWS + ["-estimator", "wc"] + OUT + ok)
    return out


def run(bin_dir, case_list):
    """key -> [exit code, stdout, stderr]"""
    import os
    got = {}
    for key, tool, args in case_list:
        assert key not in got, key
        r = subprocess.run([os.path.join(bin_dir, tool)] + args, capture_output=True, timeout=60)
        got[key] = [r.returncode, r.stdout.decode("utf-8"), r.stderr.decode("utf-8")]
    return got
