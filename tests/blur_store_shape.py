"""A catalogue of hand-built drops for the way the defocus blur writes finished tiles (the column passes of k_blur_small and
k_blur_fused_dma hand out (row, column block) with the column block fastest and store whole rows): every branch of the two
column passes, every remainder of the tile width against the four-column block, one and several loop iterations, bands,
split drops and 2-D sub-tiles whose last column is narrower than a block.

Every blurred entry is followed in table order by an in-focus drop laid over it: that neighbour's raw tile is the next thing in
the frame's arena and its footprint overlaps the blurred tile, so a store past the finished tile, or to a wrong row of it,
changes the mask.

Entries are in the format of blur_routes.CATALOGUE; the classes are found by classes(), from blur_routes.classify_drops, never
by hand arithmetic."""
import blur_routes as br

H, W = 160, 256
C1 = 1.05                           # r1 = 4, r2 = 2
C03 = 0.3                           # r1 = 1, r2 = 1

# (name, expected route, expected flags, big?, x0, y0, tw, th, c)
BLURRED = [
    # k_blur_small: one output per lane, two per lane, the copy path
    ('small_one', 'small', (), False, 8, 6, 4, 6, C03),
    ('small_two', 'small', (), False, 20, 6, 4, 12, C03),
    ('small_copy', 'small', ('row_r0',), False, 32, 6, 4, 30, 0.2),
    # ... the general branch: pw = tw + 2 r2 with every remainder, odd by odd, more than 64 blocks
    ('small_w9', 'small', (), False, 44, 8, 5, 13, C1),
    ('small_w10', 'small', (), False, 62, 8, 6, 12, C1),
    ('small_w11', 'small', (), False, 80, 8, 7, 12, C1),
    ('small_w12', 'small', (), False, 98, 8, 8, 12, C1),
    ('small_two_iters', 'small', (), False, 118, 8, 8, 20, C1),
    # k_blur_fused_dma, one sub-tile: ew = tw + 2 r2 with every remainder; fewer / more than 256 (row, block) pairs
    ('single_w20', 'fused_single', (), True, 140, 8, 16, 17, C1),
    ('single_w21', 'fused_single', (), True, 166, 8, 17, 17, C1),
    ('single_w22', 'fused_single', (), True, 194, 8, 18, 17, C1),
    ('single_w23', 'fused_single', (), True, 222, 8, 19, 17, C1),
    ('single_big', 'fused_single', (), True, 8, 60, 20, 30, br.coc_for_radius(8)),
    # ... full-width bands: odd ew with a shorter last band; a split drop
    ('bands_odd', 'fused_bands', ('partial_band',), True, 48, 60, 19, 60, br.coc_for_radius(8)),
    ('bands_split', 'fused_bands', ('split', 'zero_item', 'partial_band'), True, 90, 12, 96, 130, C1),
    # ... 2-D sub-tiles whose last column is no multiple of the block
    ('subtiles_2d', 'fused_2d', ('split', 'zero_item', 'partial_band'), True, 150, 100, 61, 4, br.coc_for_radius(20)),
]


def entries():
    """BLURRED with an in-focus neighbour behind every entry, across the middle of the blurred tile."""
    out = []
    for e in BLURRED:
        name, _, _, big, x0, y0, tw, th, c = e
        out.append(e)
        out.append((name + '_neighbour', 'no_blur', (), False, x0 + (tw - 5 if big else 0 if tw <= 4 else tw) // 2, y0 + 1, 4, max(th - 2, 3), 0.0))
    return out


def particles():
    return br.catalogue_particles(entries(), H, W)


def classes(recs):
    """{class of the issue's list: names of the entries that reach it}."""
    out = {}

    def put(k, name):
        out.setdefault(k, []).append(name)
    for (name, *_), r in zip(entries(), recs):
        if not r['live'] or r['r1'] == 0:
            continue
        ew, eh, r2 = r['ew'], r['eh'], r['r2']
        if r['route'] == 'small':
            nh = ((ew + 3) // 4) * eh
            if r2 == 0:
                put('small_copy', name)
            elif nh <= 16:
                assert ew * eh <= 64
                put('small_one_per_lane', name)
            elif nh <= 32:
                put('small_two_per_lane', name)
            if r2 > 0 and nh > 32:
                put('small_general_w%d' % (ew % 4), name)
                if ew % 2 and eh % 2:
                    put('small_general_odd_odd', name)
                if nh > 64:
                    put('small_general_two_iterations', name)
        elif r['route'] in br.FUSED:
            wo, ho = r['wo'], r['ho']
            if r['route'] == 'fused_single':
                put('single_w%d' % (ew % 4), name)
                put('single_more_than_256_pairs' if ((wo + 3) // 4) * ho > 256 else 'single_fewer_than_256_pairs', name)
            elif r['route'] == 'fused_bands':
                if ew % 2 and 'partial_band' in r['flags']:
                    put('bands_odd_partial', name)
                if 'split' in r['flags']:
                    put('bands_split', name)
            elif (ew % wo) % 4:
                put('2d_last_column_not_a_block', name)
    return out


REQUIRED = (['small_copy', 'small_one_per_lane', 'small_two_per_lane', 'small_general_odd_odd', 'small_general_two_iterations'] +
            ['small_general_w%d' % k for k in range(4)] + ['single_w%d' % k for k in range(4)] +
            ['single_more_than_256_pairs', 'single_fewer_than_256_pairs', 'bands_odd_partial', 'bands_split', '2d_last_column_not_a_block'])
