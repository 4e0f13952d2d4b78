"""Inputs of the bulk sampler fixtures (tests/golden/sampler_bulk.npz, gumbel_bulk.npz), regenerated from the chunk index alone so
that only the reference's TOKENS need to be stored.  Used by tests/golden/make_golden.py (which runs the reference's sampling chain on them)
and by the parity tests.  CPU torch generators: identical on every machine with this torch build."""
import torch

BULK_CHUNKS, BULK_ROWS, BULK_V = 48, 512, 16384
BULK_PARAMS = [(250, 0.92, 1.0), (100, 0.8, 1.3), (None, 0.95, 0.9), (50, None, 1.0), (None, None, 1.0), (250, 0.92, 0.7)]
BULK_DELTA, BULK_GAMMA = 2.0, 0.25


def bulk_rows(c):
    """Chunk c: context tokens [B,1], logits [B,V], (top_k, top_p, temperature), watermark on/off."""
    g = torch.Generator().manual_seed(77000 + c)
    ctx = torch.randint(0, BULK_V, (BULK_ROWS, 1), generator=g)
    lg = torch.randn(BULK_ROWS, BULK_V, generator=g) * [1.0, 10.0, 40.0][c % 3]
    kind = (c // 3) % 4
    if kind == 2:
        lg = torch.round(lg * 2.0) / 2.0             # tie-heavy rows: many exactly equal logits
    elif kind == 3:
        lg = lg.bfloat16().float()                    # bf16-valued logits: ties in the low mantissa bits
    top_k, top_p, T = BULK_PARAMS[c % len(BULK_PARAMS)]
    use_wm = (c % 8) != 7
    return ctx, lg, top_k, top_p, T, use_wm


GUM_BULK_ROWS = 9
GUM_BULK_V = (37, 1000, 1024, 16383, 16384)
GUM_BULK_SCALES = (1.0, 3.0, 10.0, 40.0)
GUM_BULK_KINDS = ("plain", "half_integer", "bf16")
# (T, top_p, top_k).  The last one sets both cuts: engine.py takes top-p then, and nothing else in the list tells which.
GUM_BULK_SETTINGS = ((1.0, 0.0, 0), (0.7, 0.0, 0), (1.0, 0.0, 50), (1.0, 0.9, 0), (0.8, 0.5, 0), (1.0, 0.0, 1), (1.3, 0.95, 0),
                     (1.0, 1.0, 0), (1.0, 0.0, 250), (0.9, 0.0, 10 ** 6), (1.0, 0.9, 50))
GUM_BULK_CHUNKS = len(GUM_BULK_SETTINGS) * len(GUM_BULK_V) * len(GUM_BULK_SCALES) * len(GUM_BULK_KINDS)      # 660 x 9 = 5 940 rows


def gumbel_bulk_case(c):
    """Chunk c -> (V, scale, kind, (T, top_p, top_k)): the setting varies fastest, then V, the scale, the kind."""
    n_s, n_v, n_sc = len(GUM_BULK_SETTINGS), len(GUM_BULK_V), len(GUM_BULK_SCALES)
    return (GUM_BULK_V[(c // n_s) % n_v], GUM_BULK_SCALES[(c // (n_s * n_v)) % n_sc], GUM_BULK_KINDS[c // (n_s * n_v * n_sc)],
            GUM_BULK_SETTINGS[c % n_s])


def gumbel_bulk_rows(c):
    """Chunk c of the Gumbel-key bulk fixture (tests/golden/gumbel_bulk.npz): logits float32 [B, V], window hashes int64 [B],
    (T, top_p, top_k).  Row 0 of every chunk carries one of the edge hashes (0, 2^31 - 2, one above 2^32, a negative one)."""
    V, scale, kind, setting = gumbel_bulk_case(c)
    g = torch.Generator().manual_seed(55000 + c)
    lg = torch.randn(GUM_BULK_ROWS, V, generator=g) * scale
    if kind == "half_integer":
        lg = torch.round(lg * 2.0) / 2.0             # tie-heavy rows: many exactly equal logits
    elif kind == "bf16":
        lg = lg.bfloat16().float()                    # bf16-valued logits: ties in the low mantissa bits
    h = torch.randint(0, 2 ** 31 - 1, (GUM_BULK_ROWS,), generator=g)
    h[0] = (0, 2 ** 31 - 2, 2 ** 32 + 5 + c, -7 - c)[c % 4]
    return lg, h, setting


def bulk_noise(c):
    """The Exp(1) noise torch.multinomial draws for chunk c (torch.manual_seed(88000 + c) precedes the call)."""
    torch.manual_seed(88000 + c)
    return torch.empty(BULK_ROWS, BULK_V).exponential_(1)
