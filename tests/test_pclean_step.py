"""The clean panel selection's step file (krisp_amd/csrc/pclean_step.inc: the forward and backward walks over the site store,
the owners' lookups, the fate words) without a GPU.  It is plain C++ for host and device; here it is built into a stand-alone
program (tests/pclean_step_check.cpp) with -fsanitize=address,undefined, run over exact-size heap buffers on the planted sets
of panel_clean_cases.py and compared with the reference: the walks with multiplex_reference's products, site for site
(the site at position 0 and the last site of the store among them), the marks with panel_clean_reference's P.  The program
is never loaded into Python."""
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import panel_clean_cases as CC                                             # noqa: E402
import panel_clean_reference as ref                                        # noqa: E402
from multiplex_reference import ref_products                               # noqa: E402

PLANTED = [n for n in CC.SETS if not n.startswith(("random_", "shared_"))] + ["random_65", "shared_300"]


def _compilers():
    found = [shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
    return [c for c in found if c and os.path.exists(c)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/pclean_step_check.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, every report fatal"""
    compilers = _compilers()
    if not compilers:
        pytest.skip("neither g++ nor clang++ is installed")
    exe = str(tmp_path_factory.mktemp("pclean_step") / "pclean_step_check")
    said = []
    for cxx in compilers:
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, os.path.join(HERE, "pclean_step_check.cpp")], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        said.append(f"{cxx}: {r.stderr[-2000:]}")
    pytest.fail("no compiler built the sanitized program:\n" + "\n".join(said))


def _model(name):
    """a set as the program reads it, and what the reference says of it"""
    c = CC.case(name)
    texts, rows = ref.table(c["templates"], c["pairs"])
    T = len(texts)
    lens = [len(t) for t in texts]
    eoff = [0]
    for n in lens:
        eoff += [eoff[-1] + n, eoff[-1] + 2 * n]
    store = ref.store(c["files"], c["omit"], texts, c["M"])
    index = {(fi, pos, e): i for i, (fi, pos, e, _mm, _em, _u) in enumerate(store)}
    pairs = set()                                                          # (opening site, closing site) of every product
    for fi, text in enumerate(c["files"]):
        for s1, length, a, b, *_ in ref_products(text, c["omit"], texts, c["M"], c["max_product"]):
            pairs.add((index[(fi, s1, 2 * a)], index[(fi, s1 + length - lens[b], 2 * b + 1)]))
    own = ref.owners(rows, T)
    ooff = [0]
    for o in own:
        ooff.append(ooff[-1] + len(o))
    head = [T, min(lens), c["max_product"], len(rows)] + eoff + [len(store)]
    for _fi, pos, e, _mm, _em, u in store:
        head += [pos, e, u]
    head += [ooff[-1]] + ooff + [x for o in own for x in o] + [r for row in rows for r in row]
    return dict(c=c, T=T, rows=rows, store=store, pairs=pairs, own=own, head=head,
                P=ref.product_pairs(c["files"], c["omit"], texts, c["M"], c["max_product"]))


def _run(program, tmp_path, numbers):
    path = str(tmp_path / "input.txt")
    with open(path, "w") as f:
        f.write(" ".join(str(int(x)) for x in numbers) + "\n")
    r = subprocess.run([program, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    out = r.stdout.split("\n")
    assert out[-1] == ""
    return [ln.split(" ") for ln in out[:-1]]


@pytest.mark.parametrize("name", PLANTED)
def test_the_walks_find_the_reference_products_site_for_site(name, program, tmp_path):
    m = _model(name)
    ns = len(m["store"])
    got = _run(program, tmp_path, m["head"] + [1])
    assert len(got) == 2 * (ns + 2)
    fwd, bwd = set(), set()
    for ln in got:
        i, js = int(ln[1]), [int(x) for x in ln[2:]]
        if ln[0] == "f":
            assert js == sorted(js)                                           # in store order
            fwd |= {(i, j) for j in js}
        else:
            assert ln[0] == "b" and js == sorted(js, reverse=True)
            bwd |= {(j, i) for j in js}
    assert fwd == m["pairs"] and bwd == m["pairs"]
    assert not got[2 * ns][2:] and not got[2 * ns + 3][2:]                  # nothing past the store
    print(name, "sites", ns, "products", len(m["pairs"]))
    if m["c"]["planted_cross"] or name in ("self_first", "palindrome", "all_self"):
        assert m["pairs"]
    if name == "cross_backward_at_0":
        assert (0, 1) in m["pairs"] and m["store"][0][1] == 0                   # the site at position 0, found walking backward
    if name == "file_boundary":
        last0 = max(i for i, s in enumerate(m["store"]) if s[0] == 0)
        assert m["store"][last0 + 1][0] == 1 and not any(last0 in p for p in m["pairs"])
        a, b = m["store"][last0], m["store"][last0 + 1]
        assert a[5] != b[5] and b[1] >= a[1] + 12 and b[1] - a[1] < 300       # units alone keep the two sites apart
    if name == "next_block":
        assert (255, 256) in m["pairs"] and (511, 512) in m["pairs"]
    assert any(ns - 1 in p for p in m["pairs"]) or name not in ("by_2", "three_owners")     # the last site of the store


@pytest.mark.parametrize("name", PLANTED)
def test_the_marks_are_the_reference_verdicts(name, program, tmp_path):
    m = _model(name)
    rows, P, n = m["rows"], m["P"], len(m["rows"])
    selfp = [any((x, x) in P for x in rows[c]) for c in range(n)]
    cmds, want = [2], [["self"] + [str(5 if s else 0) for s in selfp]]
    members, fates, _ = CC.expected(name)
    for mem in list(range(min(n, 6))) + [mb["position"] for mb in members]:
        number = 1 + mem % 7
        # the fates a round meets: earlier candidates settled, some later ones dropped by this round's k_panel_round
        init = [5 if selfp[c] else (1 | (3 << 8)) if c < mem and c % 2 else (2 | (number << 8)) if c > mem and c % 5 == 4 else 0
                for c in range(n)]
        after = list(init)
        for c in range(mem + 1, n):
            crosses = any((x, y) in P or (y, x) in P for x in rows[mem] for y in rows[c])
            if init[c] == 0 and crosses:
                after[c] = 4 | (number << 8)
        cmds += [3, mem, number] + init
        want.append(["cross"] + [str(x) for x in after])
    for t in list(range(m["T"])) + [m["T"], m["T"] + 9, 0xffffffff]:
        cmds += [4, t]
        want.append(["own"] + [str(x) for x in (m["own"][t] if t < m["T"] else [])])
    for c in (0, n - 1, n, 0xffffffff):
        cmds += [5, c]
        want.append(["fate", str(7 if c < n else 0xffffffff)])
    got = _run(program, tmp_path, m["head"] + cmds)
    assert got == want, next((g, w) for g, w in zip(got, want) if g != w)
    # the reference's own fates 5 are the self marks
    assert [f == (5, 0) for f in fates] == selfp


def test_the_step_file_is_plain():
    step = open(os.path.join(os.path.dirname(HERE), "krisp_amd", "csrc", "pclean_step.inc")).read()
    for word in ("threadIdx", "__shared__", "__global__", "hipLaunch", "atomic"):
        assert word not in step, word
