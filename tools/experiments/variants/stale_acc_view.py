# dhtgpu_write_ids without its `acc.stale = true` line: the accept mask's view keeps the ids it was compacted from
# (same n, same mask: every read stays in bounds).  The view_index- and bmap-write_ids_* rows must fail on it.
# A test-sensitivity variant for tools/experiments/build_variant.sh: it changes no size, bound or pointer, and no
# test loads it (profiles/r14/sequences/notes.txt records the runs).
s = open("api.hip").read()
a = '    if (c->acc.has_mask) c->acc.stale = true;\n    if (int r = upload_ids(c, ids20, m, c->planes.as<uint32_t>() + first, c->stride)) return r;\n'
assert s.count(a) == 1
s = s.replace(a, '    if (int r = upload_ids(c, ids20, m, c->planes.as<uint32_t>() + first, c->stride)) return r;\n')
open("api.hip", "w").write(s)
