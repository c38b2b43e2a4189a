"""The host side launches every kernel through one checked helper (kmernator_amd/csrc/kmr_host.hpp: launch_status, and LAUNCH over it).

hipLaunchKernelGGL therefore stands in exactly one place, and hipGetLastError only in kmr_host.hpp (the helper, and dev_malloc, which
clears the error of an allocation it is about to try again) and at the few sites listed below that drop an error on purpose.  A launch
written out by hand, or a check of "whatever failed last" behind a group of launches, brings back what the helper removed: a failed
launch reported under the name of a later call, and a reader who has to work out per site whether a launch is checked at all.

The helper asks for the error itself, so a result of it that nobody looks at is a launch that is never checked: launch_status is used
only inside a condition, an assignment or another call, and a lambda that launches is never called as a statement of its own.

No GPU and no build: the sources are read as text, comments removed.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmernator_amd", "csrc")

# Sites outside kmr_host.hpp that may name hipGetLastError: (file, text the line holds, why the error is dropped there)
SWALLOWED = [
    ("kmr_api.hip", "h->arena.alloc(",
     "arena_reset: the finalize arena could not be brought to size; temporaries are then allocated on the side, the sticky error is cleared"),
    ("kmr_api.hip", "h->lut.alloc(bytes)",
     "lut_of: no memory for the lookup accelerator; the callers search the buckets, the sticky error is cleared"),
    ("kmr_api.hip", "table clear failed",
     "kmr_create: there is no handle to report to yet; the error's text goes into the creation error"),
]


def _strip(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)      # (line numbers stay)
    return re.sub(r"//[^\n]*", "", text)


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp")):
            yield name, _strip(open(os.path.join(CSRC, name)).read()).split("\n")


def _lines_with(word):
    return [(name, i + 1, line.strip()) for name, lines in _sources() for i, line in enumerate(lines) if word in line]


def test_one_launch_site():
    sites = _lines_with("hipLaunchKernelGGL")
    assert [(n, l) for n, _, l in sites if n != "kmr_host.hpp"] == [], "kernels are launched through LAUNCH / launch_status (kmr_host.hpp)"
    assert len(sites) == 1, sites
    assert sum(line.count("hipLaunchKernelGGL") for _, _, line in sites) == 1


def test_last_error_only_where_listed():
    used = set()
    for name, lineno, line in _lines_with("hipGetLastError"):
        if name == "kmr_host.hpp":
            continue
        hits = [i for i, (f, text, _) in enumerate(SWALLOWED) if f == name and text in line]
        assert len(hits) == 1, "%s:%d names hipGetLastError outside the launch helper: %s" % (name, lineno, line)
        assert hits[0] not in used, "%s:%d: a second site of %r" % (name, lineno, SWALLOWED[hits[0]][1])
        used.add(hits[0])


def _body(text, brace):
    """text of the braces that open at text[brace]"""
    depth = 0
    for j in range(brace, len(text)):
        depth += text[j] == "{"
        depth -= text[j] == "}"
        if depth == 0:
            return text[brace:j + 1]
    raise AssertionError("unbalanced braces")


def test_no_launch_result_is_dropped():
    for name, lines in _sources():
        if name == "kmr_host.hpp":
            continue
        text = "\n".join(lines)
        # launch_status stands inside a condition, an assignment or a call: what precedes it on its line ends in "(", "&&", "||", "=" or "!"
        for i, line in enumerate(lines):
            for m in re.finditer(r"\blaunch_status\(", line):
                before = line[:m.start()].rstrip()
                assert re.search(r"(\(|&&|\|\||=|!)$", before), "%s:%d: the result of launch_status is not looked at: %s" % (name, i + 1, line.strip())
        # a named lambda that launches hands its status back: no call of it is a statement of its own
        for m in re.finditer(r"\bauto (\w+) = \[[^\]]*\]\s*\([^)]*\)[^{;]*\{", text):
            if not re.search(r"\b(LAUNCH|launch_status)\(", _body(text, m.end() - 1)):
                continue
            bare = [j + 1 for j, line in enumerate(lines) if re.match(r"\s*(else\s+|if \([^;]*\)\s+)?%s\(" % re.escape(m.group(1)), line)]
            assert not bare, "%s: the lambda %s launches a kernel and its result is dropped at line(s) %s" % (name, m.group(1), bare)
