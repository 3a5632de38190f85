"""Critical path of k_chol_tiles from a trace written by `SE2GPU_BA_CHOL_TRACE=1 python tools/chol_trace.py 200 2> trace.txt`:
    python tools/chol_trace_summary.py trace.txt
Walks back from the tile task that publishes last through the producer that published last among the entries it polls in
earnest: the end of its dependency list, which is in depth order - one entry on a plain chain, the last columns of both arcs at
the junction in front of the first separator column (`choleager` lines; a trace without them has one such entry per task)."""
import sys

lines = [l.split() for l in open(sys.argv[1])]
rows = [l for l in lines if l and l[0] == "choltrace"]
eager = {int(l[1]): list(map(int, l[2:])) for l in lines if l and l[0] == "choleager"}   # (the same for every solve of the trace)
n = len(rows) // 3          # tools/chol_trace.py solves three times; the last solve is analysed
T = {}
for r in rows[-n:]:
    t, i, kind, j, dep = map(int, r[1:6])
    T[(i, kind, j)] = (dep, list(map(int, r[6:])), eager.get(t, [dep]))
tiles = {k: v for k, v in T.items() if k[1] != 2}
print("tile tasks %d, x tasks %d, last tile published at %.1f us, last x task started at %.1f us" % (
    len(tiles), len(T) - len(tiles), max(v[1][5] for v in tiles.values()) / 100, max(v[1][0] for k, v in T.items() if k[1] == 2) / 100))
k = max(tiles, key=lambda k: tiles[k][1][5])
path = []
while True:
    dep, st, last = tiles[k]
    if dep < 0:
        path.append((k, dep, st))
        break
    i, kind, j = k
    cands = []
    for e in last:
        m, hasT = e & 0x7fff, e >> 15
        cs = [(j, 0, m)]
        if hasT: cs.append((i, kind, m))
        cs = [c if c in tiles else (c[0], 1, c[2]) for c in cs]   # the diagonal task publishes R(m, m)
        cands += [(c, e) for c in cs if c in tiles]
    if not cands:
        path.append((k, dep, st))
        break
    nxt, dep = max(cands, key=lambda c: tiles[c[0]][1][5])
    path.append((k, dep, st))
    k = nxt
path.reverse()
prev = None
tot = dict(flag=0, loads=0, mfma=0, staging=0, elim=0, publish=0)
for (k, dep, st) in path:
    f = (st[1] - prev) / 100 if prev is not None else 0.0
    ld = (st[7] - st[1]) / 100 if dep >= 0 else 0.0
    mf = (st[2] - st[7]) / 100 if dep >= 0 else 0.0
    sg, el, pb = (st[3] - st[2]) / 100, (st[4] - st[3]) / 100, (st[5] - st[4]) / 100
    for key, v in zip(tot, (f, ld, mf, sg, el, pb)): tot[key] += v
    print(f"tile ({k[0]:2d},{k[2]:2d}){'R' if k[1] else 'A'} after column {dep & 0x7fff if dep >= 0 else -1:2d}: last slab flag {f:5.2f}  its loads + staging {ld:5.2f}  "
          f"rest of the products {mf:5.2f}  to LDS {sg:5.2f}  elimination {el:5.2f}  publish {pb:5.2f}   [us]  published at {st[5] / 100:6.1f}")
    prev = st[5]
print("chain of %d tasks: " % len(path) + "  ".join(f"{k} {v:.1f}" for k, v in tot.items()))
