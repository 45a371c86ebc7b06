"""The clean panel selection's definition in plain loops, the yardstick of test_panel_clean_cases.py,
test_pclean_step.py, test_panel_clean_host.py, test_gpu_panel_clean.py and test_gpu_panel_clean_cli.py.  Same locus, the
cross figure and the primers are panel_reference's, the site and the product multiplex_reference's: imported, not restated.
Nothing of krisp_amd/ is imported.

The table: the distinct primer texts of ALL candidates (a candidate's two texts are its left_sequence and right_sequence),
ordered by their bytes.  P: the ordered pairs of texts (a, b) with a product -- a opens, b closes -- in at least one file;
a product never spans two files or two records.  A candidate is self-priming when (x, x) is in P for one of its texts x: its
fate is (5, 0) before the first round.  A candidate crosses a member when (x, y) or (y, x) is in P for a text x of the member
and a text y of the candidate.  After a member is accepted every later candidate still alive is tested against it: same
locus -> 2, else clash -> 3, else cross -> 4; the running figures are updated where panel_reference.select updates them.
"""
from multiplex_reference import ref_products, ref_sites
from panel_reference import cross_figure, primers, same_locus


def table(templates, pairs):
    """-> (texts: the distinct primer texts as bytes, ordered; rows: (left row, right row) per candidate)"""
    oligos = [primers(t, p) for t, p in zip(templates, pairs)]
    texts = sorted({x.encode() for o in oligos for x in o})
    at = {x: i for i, x in enumerate(texts)}
    return texts, [(at[a.encode()], at[b.encode()]) for a, b in oligos]


def owners(rows, T):
    """owners[t] = the positions of the candidates one of whose texts is row t, ascending, each once"""
    out = [[] for _ in range(T)]
    for i, (a, b) in enumerate(rows):
        out[a].append(i)
        if b != a:
            out[b].append(i)
    return out


def store(files, omit, texts, M):
    """the sites of every file with their record numbers: [(file, pos, entry, mismatches, end_mismatches, unit)], a file's
    sites by (pos, entry); unit = the records of the files before (a file has its separators + 1) + the separators before pos"""
    out, base = [], 0
    for fi, text in enumerate(files):
        text = bytes(text)
        for pos, e, mm, em in ref_sites(text, omit, texts, M):
            out.append((fi, pos, e, mm, em, base + text.count(b"\n", 0, pos)))
        base += text.count(b"\n") + 1
    return out


def product_pairs(files, omit, texts, M, max_product):
    """P: {(a, b)}: text a opens and text b closes a product in at least one file"""
    P = set()
    for text in files:
        for row in ref_products(bytes(text), omit, texts, M, max_product):
            P.add((row[2], row[3]))
    return P


def select(templates, pairs, size, max_sec, files, omit, M, max_product):
    """-> (members: dicts position, cross_any, cross_end, dropped [same locus, clash], in order of acceptance;
    fates: (fate, by) per candidate; drops: [self-priming candidates, dropped as cross by member 1, by member 2, ...])"""
    n = len(templates)
    oligos = [primers(t, p) for t, p in zip(templates, pairs)]
    texts, rows = table(templates, pairs)
    P = product_pairs(files, omit, texts, M, max_product)
    fate = [(0, 0)] * n
    for c in range(n):
        if any((x, x) in P for x in rows[c]):
            fate[c] = (5, 0)
    drops = [sum(1 for f in fate if f[0] == 5)]
    running = [(0, 0)] * n
    members = []
    while len(members) < size:
        alive = [i for i in range(n) if fate[i] == (0, 0)]
        if not alive:
            break
        m = alive[0]
        number = len(members) + 1
        fate[m] = (1, number)
        member = {"position": m, "cross_any": running[m][0], "cross_end": running[m][1], "dropped": [0, 0]}
        members.append(member)
        drops.append(0)
        for c in alive[1:]:
            if same_locus(templates[m], templates[c]):
                fate[c] = (2, number)
                member["dropped"][0] += 1
                continue
            a, e = cross_figure(oligos[c], oligos[m])
            running[c] = (max(running[c][0], a), max(running[c][1], e))
            if a > max_sec or e > max_sec:
                fate[c] = (3, number)
                member["dropped"][1] += 1
                continue
            if any((x, y) in P or (y, x) in P for x in rows[m] for y in rows[c]):
                fate[c] = (4, number)
                drops[number] += 1
    return members, fate, drops
