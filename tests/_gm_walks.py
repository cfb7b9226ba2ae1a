"""What tests/test_gconv_mfma_plan_cpu.py and tests/test_gpu_gconv_mfma_walks.py share: the plan of a matrix-core grouped conv
(``ops.grouped_mfma_plan``: host arithmetic, no GPU), models of what the kernels do with it that are written from the definition of
the conv and of the flat pixel index — not from the kernels' helpers —, float64 references fast enough for a few thousand channels,
and the GPU case lists with the property each case exists for (the CPU module checks those without a GPU).

Case formats are those of the three GPU modules whose helpers the new one reuses:
  fp32   ((cin_g, cout_g), G, (kernel, stride, padding), (H, W), (x layout, y layout), kind, N)
  planes (G, cin_g, cout_g, N, H, W, kernel, stride, (ph, pw))"""
import numpy as np

from pytorch_quantize_impls_amd import ops

CIN_G, COUT_G, PLANES_CIN_G = (16, 24, 32), (16, 32, 48), (16, 32)
LAYOUTS = (("nchw", "nchw"), ("nchw", "channels_last"), ("channels_last", "nchw"), ("channels_last", "channels_last"))
KINDS = ("binary", "ternary", "raw")


def out_hw(H, W, k, s, ph, pw):
    return (H + 2 * ph - k) // s + 1, (W + 2 * pw - k) // s + 1


def plan(op, ci, co, G, N, H, W, k, s, ph, pw):
    return ops.grouped_mfma_plan(op, (N, G * ci, H, W), (G * co, ci, k, k), s, (ph, pw), 1, G)


def fp32_plan(op, c):
    (ci, co), G, (k, s, p), (H, W), _lay, _kind, N = c
    return plan(op, ci, co, G, N, H, W, k, s, p, p)


def planes_plan(c):
    G, ci, co, N, H, W, k, s, (ph, pw) = c
    return plan("planes", ci, co, G, N, H, W, k, s, ph, pw)


# ---- the fp32 kernels: what a tile reads, from the definition of the conv ---------------------------------------------------------

def span(op, d0, d1, size_src, k, s, p):
    """Length of the smallest run of source rows (columns) that holds every source the destination rows [d0, d1) touch along one
    axis.  forward / grad_weight: output row r reads input rows r s - p + i, i < k, inside the input.  grad_input: input row r
    receives from every output row h with h s - p + i == r for some i < k, inside the output."""
    if op == "grad_input":
        src = [h for h in range(size_src) if any(d0 <= h * s - p + i < d1 for i in range(k))]
    else:
        src = [r * s - p + i for r in range(d0, d1) for i in range(k) if 0 <= r * s - p + i < size_src]
    return max(src) - min(src) + 1 if src else 0


def largest_box(op, pl, H, W, k, s, ph, pw):
    """Pixels of the largest bounding box any tile of the plan reads: rows and columns are independent, and the tiles are a grid."""
    Ho, Wo = out_hw(H, W, k, s, ph, pw)
    (Hs, Ws), (Hd, Wd) = ((Ho, Wo), (H, W)) if op == "grad_input" else ((H, W), (Ho, Wo))
    rows = max(span(op, r0, min(r0 + pl["TR"], Hd), Hs, k, s, ph) for r0 in range(0, Hd, pl["TR"]))
    cols = max(span(op, c0, min(c0 + pl["TC"], Wd), Ws, k, s, pw) for c0 in range(0, Wd, pl["TC"]))
    return rows * cols


def dest_map(op, H, W, k, s, ph, pw):
    return (H, W) if op == "grad_input" else out_hw(H, W, k, s, ph, pw)


# ---- the planes kernel: the register walk of a lane ------------------------------------------------------------------------------

MUTANTS = ("carry_wo", "carry_ho", "d_n", "d_ho", "d_wo")


def walk(N, Ho, Wo, pl, without=None):
    """Replay of the division-free pixel walk for every (wave, lane) at once: lane p of the wave of split sp starts at pixel
    16 sp + p, divided out once; a step adds (d_n, d_ho, d_wo) and carries wo -> ho -> n.  Returns the steps as a list of
    (flat index [splits, 16], inside the image, (n, ho, wo) registers); ``without``: the walk with one carry or one term dropped."""
    S, d_n, d_ho, d_wo = pl["splits"], pl["d_n"], pl["d_ho"], pl["d_wo"]
    if without in ("d_n", "d_ho", "d_wo"):
        d_n, d_ho, d_wo = (0 if without == name else v for name, v in (("d_n", d_n), ("d_ho", d_ho), ("d_wo", d_wo)))
    npix = N * Ho * Wo
    nxt = 16 * np.arange(S, dtype=np.int64)[:, None] + np.arange(16, dtype=np.int64)[None, :]
    first = np.where(nxt < npix, nxt, 0)
    rn, rho, rwo = first // (Ho * Wo), first % (Ho * Wo) // Wo, first % Wo
    steps = []
    for u0 in range(0, pl["units"], S):
        live = (np.arange(S) + u0 < pl["units"])[:, None]                  # the waves that still have a tile
        steps.append((nxt.copy(), (nxt < npix) & live, (rn.copy(), rho.copy(), rwo.copy())))
        nxt = nxt + 16 * S
        rwo = rwo + d_wo
        c1 = rwo >= Wo
        rwo = rwo - np.where(c1, Wo, 0)
        rho = rho + d_ho + (0 if without == "carry_wo" else c1)
        c2 = rho >= Ho
        rho = rho - np.where(c2, Ho, 0)
        rn = rn + d_n + (0 if without == "carry_ho" else c2)
    return steps


def visited(N, Ho, Wo, pl, without=None):
    """The (n, ho, wo) the walk hands to the tap loads, per (step, wave, lane), as one array; -1 where the lane has no pixel."""
    out = []
    for _flat, inside, (rn, rho, rwo) in walk(N, Ho, Wo, pl, without):
        out.append(np.where(inside[None], np.stack([rn, rho, rwo]), -1))
    return np.stack(out)


def walk_facts(N, Ho, Wo, pl):
    """(steps of the waves with the fewest / the most tiles, the wo carry fires on a pixel inside, the ho carry does)."""
    steps = walk(N, Ho, Wo, pl)
    fires = [False, False]
    for (_f, inside, (_n, ho, wo)), (_f2, inside2, _regs) in zip(steps, steps[1:]):
        both = inside & inside2
        fires[0] |= bool((both & (wo + pl["d_wo"] >= Wo)).any())
        fires[1] |= bool((both & (ho + pl["d_ho"] + (wo + pl["d_wo"] >= Wo) >= Ho)).any())
    return pl["units"] // pl["splits"], -(-pl["units"] // pl["splits"]), fires[0], fires[1]


# ---- float64 references by matrix products (exact on integers whose sums of magnitudes stay below 2^53) ----------------------------

def _cols(x, k, s, ph, pw, Ho, Wo):
    """[C, k k, Ho Wo] float64 of one image [C, H, W]: the taps in row-major order."""
    xp = np.pad(np.asarray(x, dtype=np.float64), ((0, 0), (ph, ph), (pw, pw)))
    taps = [xp[:, i:i + s * (Ho - 1) + 1:s, j:j + s * (Wo - 1) + 1:s] for i in range(k) for j in range(k)]
    return np.stack(taps, axis=1).reshape(x.shape[0], k * k, Ho * Wo)


def forward64(x, wq, bias, G, k, s, ph, pw):
    N, C, H, W = x.shape
    Cout, ci = wq.shape[:2]
    Ho, Wo = out_hw(H, W, k, s, ph, pw)
    w = np.asarray(wq, dtype=np.float64).reshape(G, Cout // G, ci * k * k)
    y = np.stack([np.matmul(w, _cols(x[n], k, s, ph, pw, Ho, Wo).reshape(G, ci * k * k, Ho * Wo)) for n in range(N)])
    y = y.reshape(N, Cout, Ho, Wo)
    return y if bias is None else y + np.asarray(bias, dtype=np.float64)[None, :, None, None]


def grad_input64(go, wq, x_shape, G, k, s, ph, pw):
    N, C, H, W = x_shape
    Cout, ci = wq.shape[:2]
    Ho, Wo = go.shape[2:]
    wt = np.asarray(wq, dtype=np.float64).reshape(G, Cout // G, ci * k * k).transpose(0, 2, 1)
    gx = np.zeros((N, C, H + 2 * ph, W + 2 * pw))
    for n in range(N):
        cols = np.matmul(wt, np.asarray(go[n], dtype=np.float64).reshape(G, Cout // G, Ho * Wo)).reshape(C, k * k, Ho, Wo)
        for t in range(k * k):
            i, j = divmod(t, k)
            gx[n, :, i:i + s * (Ho - 1) + 1:s, j:j + s * (Wo - 1) + 1:s] += cols[:, t]
    return gx[:, :, ph:ph + H, pw:pw + W]


def grad_weight64(x, go, G, ci, k, s, ph, pw):
    """(gw, grad_bias) in float64."""
    N, C, H, W = x.shape
    Cout, Ho, Wo = go.shape[1:]
    gw = np.zeros((G, Cout // G, ci * k * k))
    for n in range(N):
        cols = _cols(x[n], k, s, ph, pw, Ho, Wo).reshape(G, ci * k * k, Ho * Wo)
        gw += np.matmul(np.asarray(go[n], dtype=np.float64).reshape(G, Cout // G, Ho * Wo), cols.transpose(0, 2, 1))
    return gw.reshape(Cout, ci, k, k), np.asarray(go, dtype=np.float64).sum((0, 2, 3))


# ---- the GPU cases ------------------------------------------------------------------------------------------------------------------

# 1. multi-unit walks, forward and grad_input: every workgroup takes two or three tiles and its consecutive tiles differ in shape
#    and in patch box.  A unit is (image, tile of the image) and a workgroup steps by `splits`, so the splits (ceil(1024 / G): 7
#    at G = 147, 9 at G = 114) must not be a multiple of the 4 or 9 ragged tiles of an image — at G = 128 (8 splits over 4 tiles)
#    every workgroup would meet one tile shape only.  Batch 4 - 5, both layouts on either side, stride 1 and 2, one cin_g = 24
WALKS = (((16, 16), 147, (3, 1, 1), (9, 33), LAYOUTS[1], "binary", 4),
         ((16, 16), 147, (3, 2, 1), (13, 65), LAYOUTS[2], "ternary", 4),
         ((24, 16), 114, (3, 1, 1), (9, 33), LAYOUTS[3], "raw", 5))
# 2. the same walk in grad_weight, on an instantiation the 33-image case of tests/test_gpu_gconv_mfma_wgrad.py does not run
WGRAD_WALK = ((24, 32), 147, (3, 1, 1), (9, 33), LAYOUTS[1], "binary", 4)
# 3. the LDS budget takes rows (maps 56 wide, 32 -> 48) and columns from the first tile: {op: case}
SHRINK_ROWS = {op: ((32, 48), 2, (3, 1, 1), (8, 56), LAYOUTS[i], KINDS[i], 3) for i, op in enumerate(("forward", "grad_input", "grad_weight"))}
SHRINK_COLS = {"forward": ((32, 48), 2, (3, 2, 1), (8, 56), LAYOUTS[1], "ternary", 3),
               "grad_input": ((32, 48), 2, (3, 1, 1), (8, 32), LAYOUTS[2], "raw", 3)}
# 4. every instantiation: the channel pairs tests/test_gpu_gconv_mfma.py leaves out, 1 x 1 and 3 x 3, on its 9 x 7 map
PAIRS_LEFT = tuple((ci, co) for ci in CIN_G for co in COUT_G if (ci, co) not in ((16, 16), (24, 48), (32, 32)))
INSTANCES = tuple((ch, 8 + i % 2, geo, (9, 7), LAYOUTS[(2 * i + j) % 4], KINDS[(2 * i + j) % 3], 2)
                  for i, ch in enumerate(PAIRS_LEFT) for j, geo in enumerate(((1, 1, 0), (3, 1, 1))))
WGRAD_INSTANCES = tuple(((ci, co), 8 + i % 2, geo, (9, 7), LAYOUTS[i % 4], "binary", 2)
                        for i, (ci, co, geo) in enumerate((ci, co, geo) for ci in CIN_G for co in COUT_G for geo in ((1, 1, 0), (3, 2, 1))))
PLANES_INSTANCES = ((9, 16, 16, 3, 5, 17, 1, 2, (0, 0)), (10, 16, 48, 3, 5, 17, 1, 2, (0, 0)), (9, 32, 32, 3, 5, 17, 1, 2, (0, 0)),
                    (10, 32, 16, 3, 5, 17, 1, 2, (0, 0)), (9, 32, 16, 3, 5, 17, 3, 2, (1, 0)))
# 5. the planes walk: two or three steps a wave, all three increments, both carries, a partial last tile; G % 4 != 0 in the last
PLANES_WALKS = ((128, 16, 16, 50, 5, 5, 1, 1, (0, 0)), (256, 32, 16, 23, 5, 5, 1, 1, (0, 0)), (130, 16, 32, 49, 3, 7, 1, 1, (0, 0)))


def unit_walks(op, c):
    """Per workgroup (split) of a group, the tiles it takes in order, from the plan and the definition of the conv: unit u is tile
    u % tiles of image u // tiles, tiles row-major; a tile is (rows, columns, rows of its patch box, columns of its patch box)."""
    pl = fp32_plan(op, c)
    (k, s, p), (H, W) = c[2], c[3]
    Ho, Wo = out_hw(H, W, k, s, p, p)
    (Hs, Ws), (Hd, Wd) = ((Ho, Wo), (H, W)) if op == "grad_input" else ((H, W), (Ho, Wo))
    tiles = []
    for r0 in range(0, Hd, pl["TR"]):
        for c0 in range(0, Wd, pl["TC"]):
            r1, c1 = min(r0 + pl["TR"], Hd), min(c0 + pl["TC"], Wd)
            tiles.append((r1 - r0, c1 - c0, span(op, r0, r1, Hs, k, s, p), span(op, c0, c1, Ws, k, s, p)))
    assert len(tiles) == pl["tiles_r"] * pl["tiles_c"]
    return [[tiles[u % len(tiles)] for u in range(split, pl["units"], pl["splits"])] for split in range(pl["splits"])]


def multi_unit(op, c):
    """The property of the walk cases, from the plan alone: two trips and more for every workgroup over ragged 2 x 2 (or more) tiles;
    in EVERY workgroup some tile follows one of another shape (rows x columns) with another patch box, and among the workgroups a
    smaller tile follows a larger one (what a remnant of the previous tile in the LDS patch or the tables would need) and a larger
    one a smaller."""
    pl = fp32_plan(op, c)
    (k, s, p), (H, W) = c[2], c[3]
    Hd, Wd = dest_map(op, H, W, k, s, p, p)
    walks = unit_walks(op, c)
    pairs = [list(zip(w, w[1:])) for w in walks]
    differ = all(any(a[:2] != b[:2] and a[2:] != b[2:] for a, b in pw) for pw in pairs)
    shrinks = any(b[0] * b[1] < a[0] * a[1] and b[2] * b[3] < a[2] * a[3] for pw in pairs for a, b in pw)
    grows = any(b[0] * b[1] > a[0] * a[1] and b[2] * b[3] > a[2] * a[3] for pw in pairs for a, b in pw)
    return (pl["units"] >= 2 * pl["splits"] + 1 and pl["tiles_r"] >= 2 and pl["tiles_c"] >= 2 and Hd % pl["TR"] != 0
            and Wd % pl["TC"] != 0 and c[6] >= 3 and differ and shrinks and grows)
