"""The panel pass's definition in plain loops over Python strings, the yardstick of test_panel_cases.py,
test_panel_host.py, test_panel_step.py, test_gpu_panel.py and test_gpu_panel_cli.py.  No table, no key, no early exit that
the definition does not have.  It shares with the package the integer tables of krisp_amd/thermo.py -- through
design_reference.duplex_figure, which is imported, not restated -- and nothing else.
"""
import functools

from design_reference import duplex_figure, rc

WINDOW = 16
# (a figure is a function of the two texts alone: a set whose primers repeat asks for each once)
_figure = functools.lru_cache(maxsize=None)(duplex_figure)


def windows(t):
    """the windows of 16 bases of the text t; one that holds a letter other than A, C, G, T is no window"""
    return {t[i:i + WINDOW] for i in range(len(t) - WINDOW + 1) if not set(t[i:i + WINDOW]) - set("ACGT")}


def same_locus(a, b):
    """do the templates a and b share a window, b read on either strand?"""
    wa = windows(a)
    return any(w in wa or rc(w) in wa for w in windows(b))


def primers(template, pair):
    """(left, right) of a candidate, both 5'->3', as the CSV's left_sequence / right_sequence"""
    ls, ln, rs, rn = pair
    return template[ls:ls + ln], rc(template[rs:rs + rn])


def cross_figure(cand, member):
    """(any, end): the greatest figures over the four (x, y), x a primer of the candidate, y one of the member"""
    any_, end = 0, 0
    for x in cand:
        for y in member:
            a, e = _figure(x, y)
            any_, end = max(any_, a), max(end, e)
    return any_, end


def select(templates, pairs, size, max_sec):
    """templates: str rows, pairs: (ls, ln, rs, rn) rows, in the order the selection goes by ->
    (members: dicts position, cross_any, cross_end, dropped [same locus, clash], in order of acceptance;
     fates: (fate, by) per candidate)"""
    n = len(templates)
    oligos = [primers(t, p) for t, p in zip(templates, pairs)]
    fate = [(0, 0)] * n
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
    return members, fate
