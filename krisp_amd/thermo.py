"""The integer thermodynamic model of `krisp_fasta --design-primers`, held once: the library receives these
integers in kr_design_table, the brute-force reference of the tests imports the same tables, nothing else restates them.

Enthalpy in cal/mol, entropy in 0.001 cal/(mol K), temperatures in mK.  Nearest-neighbour steps: SantaLucia 1998 unified,
read 5'->3' on the oligo.  Tm_mK = (dH * 10^6) // dS_total, both negative, int64, floor division.  This is NOT Primer3's
model: no `thal` alignment, no gapped or mismatched duplexes; the hairpin figure of --hairpins (LOOP_DS below)
is a model of this project's own too.
"""
import ctypes
import math

BASES = "ACGT"                                   # the codes 0 .. 3 of the tables; the complement of code b is 3 - b

_STEPS = {                                       # step: (dH, dS); a step and its reverse complement are one entry
    ("AA", "TT"): (-7900, -22200), ("AT",): (-7200, -20400), ("TA",): (-7200, -21300),
    ("CA", "TG"): (-8500, -22700), ("GT", "AC"): (-8400, -22400), ("CT", "AG"): (-7800, -21000),
    ("GA", "TC"): (-8200, -22200), ("CG",): (-10600, -27200), ("GC",): (-9800, -24400), ("GG", "CC"): (-8000, -19900),
}
NN_DH = [0] * 16                                 # [4 * code(x) + code(y)] of the step xy
NN_DS = [0] * 16
for _names, (_h, _s) in _STEPS.items():
    for _n in _names:
        NN_DH[4 * BASES.index(_n[0]) + BASES.index(_n[1])] = _h
        NN_DS[4 * BASES.index(_n[0]) + BASES.index(_n[1])] = _s
TERM_DH = [2300, 100, 100, 2300]                 # per terminal base: A/T +2300 / +4100, G/C +100 / -2800
TERM_DS = [4100, -2800, -2800, 4100]
SYM_DS = -1400                                   # an oligo equal to its own reverse complement
SALT_DS = round(368 * math.log(0.05))            # per step: 50 mM monovalent
CONC_DS = round(1000 * 1.987 * math.log(50e-9 / 4))      # 50 nM, two different strands
CONC_SELF_DS = round(1000 * 1.987 * math.log(50e-9))     # ... a self-complementary one


# --hairpins: a hairpin loop's free energy at 37 degrees C in cal/mol by the number of bases the innermost
# pair encloses.  THESE NUMBERS ARE THE DEFINITION: they follow SantaLucia & Hicks 2004 as remembered and were not checked
# against the paper.  Between two listed lengths: linear, in integers, floor; above 30: 40 per base.  The loop's enthalpy is
# 0, so its entropy is -dG / 310.15 K, here in 0.001 cal/(mol K), rounded.
LOOP_DG37 = {3: 3500, 4: 3500, 5: 3300, 6: 4000, 7: 4200, 8: 4300, 9: 4500, 10: 4600, 12: 5000, 14: 5100, 16: 5300, 18: 5500,
             20: 5700, 25: 6100, 30: 6300}
HAIRPIN_MIN_LOOP = 3
HAIRPIN_MAX_LOOP = 56                            # a primer of 60 bases (MAX_SIZE), two pairs


def loop_dg37(l):
    if l >= 30:
        return LOOP_DG37[30] + 40 * (l - 30)
    a = max(k for k in LOOP_DG37 if k <= l)
    b = min(k for k in LOOP_DG37 if k >= l)
    return LOOP_DG37[a] if a == b else LOOP_DG37[a] + (LOOP_DG37[b] - LOOP_DG37[a]) * (l - a) // (b - a)


# [loop length] of kr_hairpin_params: 64 entries, 3 .. 56 are read
LOOP_DS = [-((loop_dg37(l) * 100000 + 15507) // 31015) if HAIRPIN_MIN_LOOP <= l <= HAIRPIN_MAX_LOOP else 0 for l in range(64)]

ZERO_C_MK = 273150
SIZE_WEIGHT = 500                                # penalty per half base off the middle length = 1 per base, as 1000 per K
MIN_SIZE, MAX_SIZE = 10, 60                      # --primer_size the pass takes
MAX_POLY_X = 4
END_BASES = 5                                    # the 3' bases --max_end_gc counts in


def mk(celsius):
    """command-line degrees -> mK"""
    return celsius * 1000 + ZERO_C_MK


class Params(ctypes.Structure):
    """kr_design_params of include/krisp_hip.h"""
    _fields_ = ([("nn_dh", ctypes.c_int32 * 16), ("nn_ds", ctypes.c_int32 * 16), ("term_dh", ctypes.c_int32 * 4),
                 ("term_ds", ctypes.c_int32 * 4)]
                + [(n, ctypes.c_int32) for n in ("sym_ds", "salt_ds", "conc_ds", "conc_self_ds", "size_lo", "size_hi", "tm_lo",
                                                 "tm_hi", "tm_opt", "gc_lo", "gc_hi", "amp_lo", "amp_hi", "max_sec", "gc_clamp",
                                                 "max_end_gc")])


class HairpinParams(ctypes.Structure):
    """kr_hairpin_params of include/krisp_hip.h"""
    _fields_ = [("loop_ds", ctypes.c_int32 * 64)]


def hairpin_params():
    """-> HairpinParams: LOOP_DS"""
    h = HairpinParams()
    h.loop_ds[:] = LOOP_DS
    return h


def options(tm=(53, 68), gc=(40, 70), amp_size=(70, 150), primer_size=(25, 35), max_sec_tm=40, gc_clamp=1, max_end_gc=4):
    """the command line's figures as the pass's integers (temperatures in mK)"""
    return {"size_lo": primer_size[0], "size_hi": primer_size[1], "tm_lo": mk(tm[0]), "tm_hi": mk(tm[1]),
            "tm_opt": 500 * (tm[0] + tm[1]) + ZERO_C_MK, "gc_lo": gc[0], "gc_hi": gc[1], "amp_lo": amp_size[0],
            "amp_hi": amp_size[1], "max_sec": mk(max_sec_tm), "gc_clamp": gc_clamp, "max_end_gc": max_end_gc}


def refusal(tm, gc, amp_size, primer_size, max_sec_tm, gc_clamp, max_end_gc):
    """why the pass does not take these figures (one line), or None"""
    for name, r in (("--tm", tm), ("--gc", gc), ("--amp_size", amp_size), ("--primer_size", primer_size)):
        if r[1] < r[0]:
            return f"{name}: the upper bound {r[1]} lies below the lower bound {r[0]}"
    if primer_size[0] < MIN_SIZE or primer_size[1] > MAX_SIZE:
        return (f"--design-primers takes --primer_size within {MIN_SIZE} .. {MAX_SIZE} (got {primer_size[0]} .. "
                f"{primer_size[1]})")
    if not 0 <= gc_clamp <= primer_size[0]:
        return f"--gc_clamp must lie between 0 and the shortest primer, {primer_size[0]} (got {gc_clamp})"
    if max_end_gc < 0:
        return f"--max_end_gc must not be negative (got {max_end_gc})"
    if max(abs(t) for t in tm) > 1000 or abs(max_sec_tm) > 1000:
        return "--tm and --max_sec_tm are degrees Celsius between -1000 and 1000"
    return None


def params(**opts):
    """-> Params: the model and options(**opts)"""
    p = Params()
    p.nn_dh[:], p.nn_ds[:], p.term_dh[:], p.term_ds[:] = NN_DH, NN_DS, TERM_DH, TERM_DS
    p.sym_ds, p.salt_ds, p.conc_ds, p.conc_self_ds = SYM_DS, SALT_DS, CONC_DS, CONC_SELF_DS
    for k, v in options(**opts).items():
        setattr(p, k, v)
    return p


def milli(v):
    """an integer of thousandths as a decimal with three places: 1234 -> '1.234' (no float on the way)"""
    return ("-" if v < 0 else "") + f"{abs(v) // 1000}.{abs(v) % 1000:03d}"


def celsius(t_mk):
    return milli(t_mk - ZERO_C_MK)


def gc_percent(gc, n):
    """100 gc / n with three decimals, rounded half up in integers"""
    return milli((200000 * gc + n) // (2 * n))
