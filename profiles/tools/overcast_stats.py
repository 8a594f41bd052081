"""profiles/tools/overcast_stats.py RESULTS.db: per-kernel medians of a rocprofv3 kernel trace (rocpd database) of overcast_prof.py -
one line per (precision, scheme, cloud mode), the warm-up call dropped."""
import sqlite3, re, collections, statistics, sys
c = sqlite3.connect(sys.argv[1])
rows = c.execute("select name, start, end from kernels order by start").fetchall()
calls = []          # (precision, scheme, mode, {kernel: ms})
cur = None
for n, s, e in rows:
    k = re.sub(r"\(.*$", "", re.sub(r"^void\s+", "", n)).replace("geosrad::", "")
    if not k.startswith("k_"): continue
    prec = "fp64" if "double" in k else "fp32"
    base = k.split("<")[0]
    if base in ("k_chou_prep", "k_sorad_class", "k_sorad_ident"):
        scheme = "irrad" if base == "k_chou_prep" else "sorad"
        cur = [prec, scheme, "overcast" if base == "k_sorad_ident" else None, collections.OrderedDict()]
        calls.append(cur)
    if base == "k_chou_bands": cur[2] = "overcast" if "true" in k else "default"
    if base == "k_sorad_class": cur[2] = "default"
    name = base + ("<OC>" if ("true" in k) else "") if base in ("k_chou_bands", "k_sorad_cloud") else base
    cur[3][name] = cur[3].get(name, 0) + (e - s) / 1e6
groups = collections.OrderedDict()
for p, sch, mode, d in calls:
    groups.setdefault((p, sch, mode), []).append(d)
for key, L in groups.items():
    L = L[1:]               # drop the warm-up call
    names = list(L[0].keys())
    med = {n: statistics.median(d.get(n, 0) for d in L) for n in names}
    tot = statistics.median(sum(d.values()) for d in L)
    print(f"{key[0]} {key[1]:5s} {key[2]:8s} n={len(L)} total {tot:8.3f} ms | " + ", ".join(f"{n} {v:.3f}" for n, v in med.items()))
