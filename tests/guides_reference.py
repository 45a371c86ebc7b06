"""The guide pass's definition restated with Python ints and strings: every candidate, every outgroup row and
every column is walked.  It shares no code with krisp_amd/."""
BASES = "ACGT"
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
FIELDS = ("found", "strand", "start", "min_mismatches", "sum_mismatches", "gc", "candidates")


def rc(s):
    """reverse complement of a text of bases; any other letter stays what it is (it never passes the letter rule)"""
    return "".join(COMPLEMENT.get(ch, ch) for ch in reversed(s))


def candidates(rows, lo, hi, L, D, g, pam5="", pam3="", gc_lo=30, gc_hi=70, min_mismatches=1):
    """every candidate of one region that counts: (d, s, off-centre, strand, p, gc) each"""
    T, outs = rows[0], rows[1:]
    K, a, b = len(T), len(pam5), len(pam3)
    out = []
    for p in range(0, K - g + 1):
        for strand in (0, 1):
            # the footprint's columns and the two motif stretches as read on the guide's strand
            if strand == 0:
                five, three = list(range(p - a, p)), list(range(p + g, p + g + b))
            else:
                five, three = list(range(p + g + a - 1, p + g - 1, -1)), list(range(p - 1, p - b - 1, -1))
            foot = list(range(p, p + g)) + five + three
            if any(c < lo or c >= hi for c in foot):                                    # 1
                continue
            if any(T[c] not in BASES for c in foot):                                    # 2
                continue
            read = (lambda c: T[c]) if strand == 0 else (lambda c: COMPLEMENT[T[c]])
            if any(read(c) not in IUPAC[m] for c, m in zip(five, pam5.upper())):        # 3
                continue
            if any(read(c) not in IUPAC[m] for c, m in zip(three, pam3.upper())):
                continue
            proto = T[p:p + g]
            gc = sum(1 for ch in proto if ch in "GC")
            if 100 * gc < gc_lo * g or 100 * gc > gc_hi * g:                            # 4
                continue
            if any(proto[i:i + 5] == proto[i] * 5 for i in range(g - 4)):               # 5
                continue
            mm = [sum(1 for c in range(p, p + g) if o[c] in BASES and o[c] != T[c]) for o in outs]
            d = min(mm) if mm else g
            if d < min_mismatches:                                                      # 6
                continue
            out.append((d, sum(mm), abs(2 * p + g - (2 * L + D)), strand, p, gc))
    return out


def guide(rows, lo, hi, L, D, g, pam5="", pam3="", gc_lo=30, gc_hi=70, min_mismatches=1):
    """one region's record as a dict of FIELDS.  rows: texts, the template first"""
    cands = candidates(rows, lo, hi, L, D, g, pam5, pam3, gc_lo, gc_hi, min_mismatches)
    if not cands:
        return dict.fromkeys(FIELDS, 0)
    d, s, _, strand, p, gc = min(cands, key=lambda c: (-c[0], -c[1], c[2], c[3], c[4]))
    return dict(found=1, strand=strand, start=p, min_mismatches=d, sum_mismatches=s, gc=gc, candidates=len(cands))


def guides(regions, L, D, g, pam5="", pam3="", gc=(30, 70), min_mismatches=1):
    """regions: (rows, lo, hi) each -> a list of records"""
    return [guide(rows, lo, hi, L, D, g, pam5, pam3, gc[0], gc[1], min_mismatches) for rows, lo, hi in regions]
