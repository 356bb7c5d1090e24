"""A catalogue for the software pipeline of k_blur_small: a wave takes the frame's small-route drops it, it + stride, ... with
the next drop's tile and weights one drop ahead and the plan two ahead.  The other blur catalogues put about 30 drops in a
frame, so every wave takes one drop and the loop's back edge -- cur = nxt, has_next turning false in different iterations
of a workgroup's waves, the early return -- never runs.  Here one call of N_FRAMES small frames (the per-frame grid is then
capped at 64 workgroups: 256 waves) rotates three drop tables:
  A  3 * 256 + 5 small-route drops: waves 0 .. 4 run four iterations, the others three
  B  256 + 3:                        waves 0 .. 2 run two, the others one
  C  5:                              waves 0 .. 4 run one, the others leave at the first test
Every drop is a small-route drop, so entry k of a table is entry k of the frame's small list (k_lists keeps table order).

Entries are in the format of blur_routes.CATALOGUE.  census() works out, from the launch's grid formula and the classifier's
records (blur_routes.classify_drops, blur_store_shape.classes) -- never from the sizes written here -- which wave takes which
drop in which iteration and which branch of the row and column pass that drop takes."""
import blur_routes as br
import blur_store_shape as ss

H, W = 96, 160
N_FRAMES = 256
N_TABLE = (3 * 256 + 5, 256 + 3, 5)
TABLE_NAMES = 'ABC'

# (tw, th, c) of the drops, taken in turn.  13 shapes, so the drops 256 apart that one wave takes one after the other are 9
# shapes apart -- and the shapes are ordered so that any two 9 apart (mod 13) have different row radii: a prefetched drop that
# was filtered with its predecessor's weights or plan cannot come out right
C055 = 0.55                         # r1 = 2, r2 = 1
SHAPES = [
    (4, 8, C055), (5, 13, ss.C1), (5, 9, C055), (4, 24, 1.0), (6, 9, ss.C03), (4, 6, ss.C03), (8, 12, ss.C1),
    (4, 12, ss.C03), (9, 20, 1.0), (8, 20, ss.C1), (4, 30, 0.2), (6, 12, ss.C1), (4, 10, 0.2),
]


def entries(table):
    """Table `table` (0 .. 2): N_TABLE[table] small-route drops scattered over the inside of the frame."""
    out = []
    for k in range(N_TABLE[table]):
        tw, th, c = SHAPES[(k + 5 * table) % len(SHAPES)]
        x0 = 12 + (k * 37 + 11 * table) % (W - 40)
        y0 = 8 + (k * 53 + 7 * table) % (H - 48)
        out.append(('%s%d_%dx%d' % (TABLE_NAMES[table], k, tw, th), 'small', ('row_r0',) if c < 0.25 else (), False, x0, y0, tw, th, c))
    return out


def frames():
    """The three tables as the frames of one synthetic sequence."""
    return [dict(id=t, t=2000 + t, d=0, drops=br.catalogue_particles(entries(t), H, W)) for t in range(3)]


def grid_x(max_drops, n_frames):
    """Workgroups per frame of the k_blur_small launch (rr_render_frames)."""
    return min((max_drops + 3) // 4, max(64, min(2048, 16384 // n_frames)))


def row_class(r):
    """The branch of k_blur_small's row pass a classified drop takes."""
    nv4 = (((r['eh'] + 3) & ~3) >> 2) * r['tw']
    return 'row_one_per_lane' if nv4 <= 16 else 'row_two_per_lane' if nv4 <= 32 else 'row_general'


def col_class(r):
    """... and of its column pass, by blur_store_shape.classes."""
    found = set(ss.classes([r]))
    for key, name in (('small_copy', 'col_copy'), ('small_one_per_lane', 'col_one_per_lane'), ('small_two_per_lane', 'col_two_per_lane')):
        if key in found:
            return name
    assert any(k.startswith('small_general_w') for k in found), (r, found)
    return 'col_general'


ROW_CLASSES = ('row_one_per_lane', 'row_two_per_lane', 'row_general')
COL_CLASSES = ('col_one_per_lane', 'col_two_per_lane', 'col_general', 'col_copy')


def schedule(recs, max_drops, n_frames):
    """[(workgroup, wave, iteration, drop index)] of one frame: wave w of workgroup b takes entries 4 b + w + j * stride of the
    frame's small list (the small-route drops in table order), j = 0, 1, ..."""
    small = [r['i'] for r in recs if r['live'] and r['route'] == 'small']
    g = grid_x(max_drops, n_frames)
    return g, [(b, w, j, small[it]) for b in range(g) for w in range(4) for j, it in enumerate(range(4 * b + w, len(small), 4 * g))]


def census(tables, n_frames=N_FRAMES):
    """tables: the classified records of each table.  {class: [(table, workgroup, wave, iteration, drop) ...]} for the classes
    REQUIRED lists, and 'neighbours_same_r1', which must stay empty; an iteration is counted from 1."""
    out = {k: [] for k in REQUIRED + ['neighbours_same_r1']}
    max_drops = max(len(recs) for recs in tables)
    for t, recs in enumerate(tables):
        g, sched = schedule(recs, max_drops, n_frames)
        trips = {(b, w): 0 for b in range(g) for w in range(4)}
        for b, w, j, i in sched:
            trips[(b, w)] = max(trips[(b, w)], j + 1)
        for (b, w), n in trips.items():
            if n <= 4:
                out['trips_%d' % n].append((t, b, w, n, None))
        for b in range(g):
            if len({trips[(b, w)] for w in range(4)}) > 1:
                out['workgroup_mixed_trips'].append((t, b, None, None, None))
        by_wave = {}
        for b, w, j, i in sched:
            by_wave.setdefault((b, w), []).append(i)
            if j >= 1:
                out[row_class(recs[i]) + '_later'].append((t, b, w, j + 1, i))
                out[col_class(recs[i]) + '_later'].append((t, b, w, j + 1, i))
        for (b, w), idx in by_wave.items():
            for j in range(1, len(idx)):
                p, c = recs[idx[j - 1]], recs[idx[j]]
                if p['r1'] == c['r1']:
                    out['neighbours_same_r1'].append((t, b, w, j + 1, idx[j]))
                if p['r1'] != c['r1'] and row_class(p) != row_class(c) and col_class(p) != col_class(c):
                    out['neighbours_differ'].append((t, b, w, j + 1, idx[j]))
    return out


REQUIRED = (['trips_%d' % n for n in range(5)] + ['workgroup_mixed_trips'] + [k + '_later' for k in ROW_CLASSES + COL_CLASSES] +
            ['neighbours_differ'])


def drops_explaining(recs, diff, max_drops, n_frames=N_FRAMES, limit=8):
    """A short list of drops that accounts for `diff` (H x W bool, where a frame differs from its reference), with the wave and
    iteration that filtered each.  Drops overlap, so footprints alone do not tell the culprit from a neighbour lying inside it:
    a greedy cover -- take the drop whose footprint holds most of the still unexplained pixels, weighted by the share of its
    footprint that differs; strike those pixels; again."""
    where = {i: (4 * b + w, j + 1) for b, w, j, i in schedule(recs, max_drops, n_frames)[1]}
    left, out = diff.copy(), []
    cand = [r for r in recs if r['live'] and r['box'][2] > r['box'][0] and r['box'][3] > r['box'][1]]
    while left.any() and len(out) < limit:
        def gain(r):
            x0, y0, x1, y1 = r['box']
            return left[y0:y1, x0:x1].sum() * diff[y0:y1, x0:x1].mean()
        r = max(cand, key=gain)
        if gain(r) == 0:
            break
        x0, y0, x1, y1 = r['box']
        out.append('drop %d (wave %d, iteration %d, r1 %d): %d unexplained px, %.0f %% of its footprint differs'
                   % ((r['i'],) + where.get(r['i'], (-1, -1)) + (r['r1'], left[y0:y1, x0:x1].sum(), 100 * diff[y0:y1, x0:x1].mean())))
        left[y0:y1, x0:x1] = False
    return out + (['... %d px more' % left.sum()] if left.any() else [])
