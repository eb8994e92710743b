"""The optimizer kernels of two builds of libmuse_hip.so, bit for bit and launch for launch (csrc/optim.hip against the build before it):

    MUSE_HIP_LIB=/path/to/libmuse_hip.so python scripts/optim_parent_ab.py --dump FILE    # every case below -> FILE (raw bytes of every output)
    python scripts/optim_parent_ab.py --compare A B                                       # demands A == B byte for byte (exit 1 otherwise)
    MUSE_HIP_LIB=... python scripts/optim_parent_ab.py --time                             # HIP events: 5 warm-up + 20 timed launches, median per kernel
    python scripts/optim_parent_ab.py --time-lion                                         # the same method, Lion against AdamW on the same tensors

One process per library (the library is chosen when muse is imported).  Inputs come from a seeded CPU generator.  Every AdamW form runs
steps 1, 2, 3 under: the host's grad_scale 0.5; grad_scale 1/3 (no power of two: the one case where a different contraction of g*s - m
would show); the *_dev form with the device factor 1/3; `skip` at a zero counter; `skip` at a non-zero counter (every buffer, images
included, must then be unchanged to the byte - checked here, not only compared).
  flat         n = 2 * 4096 + 3, with and without the bf16 shadow                                     quads and the 3-element tail
  flat groups  the segments of tests/test_gpu_kernels.py, three groups; one call and three ranges       boundaries inside a chunk, off a multiple of 4
  multi, 6 col sizes 1 .. 3 * 8192 + 2, one tensor 4 bytes into its allocation, shadows on every second the scalar route, ragged last chunks
  multi, 7 col the same, two groups, image kind (none / bf16 copy / planes at a distance that is, and is not, a multiple of 4 / half
               copy) cycling over the tensors, every rotation of the cycle                               every image store, vector and scalar
  EMA          the same sizes, one row in copy mode, one tensor unaligned                                both modes
The whole run is ended with a traceback if it exceeds --limit seconds."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "open-muse_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from muse import ops  # noqa: E402

GROUPS3 = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05), dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
           dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1)]
SEG_SIZES, SEG_GROUP = [5000, 768, 4096, 3, 10001, 8, 4100, 12288], [0, 1, 0, 2, 0, 1, 1, 0]
MULTI_SIZES = [1, 3, 4096, 4097, 10007, 3 * 8192 + 2, 5]
UNALIGNED = 4                                  # index of the tensor that starts 4 bytes into its allocation
KINDS = ("none", "copy", "planes4", "planes_odd", "half")
VARIATIONS = ("host_half", "host_third", "dev_third", "skip_zero", "skip_set")


def raw(t):
    return t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()


def variation(name):
    """-> keyword arguments of ops.adamw_* for one variation"""
    if name == "host_half":
        return dict(grad_scale=0.5)
    if name == "host_third":
        return dict(grad_scale=1.0 / 3.0)
    if name == "dev_third":
        return dict(scale_dev=torch.tensor([1.0 / 3.0], dtype=torch.float32, device="cuda"))
    return dict(grad_scale=1.0 / 3.0, skip=torch.tensor([0 if name == "skip_zero" else 3], dtype=torch.int32, device="cuda"))


def rnd(gen, n, scale, offset=0):
    """n f32 values from the CPU generator on the device, `offset` elements into their allocation"""
    buf = torch.zeros(n + offset, dtype=torch.float32, device="cuda")
    buf[offset:].copy_(torch.randn(n, generator=gen) * scale)
    return buf[offset:]


def segments(npad):
    ends, gids, o = [], [], 0
    for sz, k in zip(SEG_SIZES, SEG_GROUP):
        o += sz
        if gids and gids[-1] == k:
            ends[-1] = o
        else:
            ends.append(o)
            gids.append(k)
    ends[-1] = npad
    return ends, gids


def image(kind, n):
    """-> (tensor that holds the image or None, table column 4, plane distance for column 6)"""
    if kind == "none":
        return None, 0, 0
    if kind == "copy":
        t = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        return t, t.data_ptr(), 0
    if kind == "half":
        t = torch.zeros(n, dtype=torch.float16, device="cuda")
        return t, t.data_ptr(), -1
    dist = (n + 3) // 4 * 4 + (1 if kind == "planes_odd" else 0)
    t = torch.zeros(dist + n, dtype=torch.bfloat16, device="cuda")
    return t, t.data_ptr(), dist


def multi_case(gen, kinds, gids, ncol):
    ts, rows = [], []
    for i, n in enumerate(MULTI_SIZES):
        off = 1 if i == UNALIGNED else 0
        p, g = rnd(gen, n, 1.0, off), rnd(gen, n, 0.1, off)
        m, v = rnd(gen, n, 0.0, off), rnd(gen, n, 0.0, off)
        img, col4, dist = image(kinds[i], n)
        ts.append((p, g, m, v, img))
        row = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), col4, n)
        rows.append(row + (gids[i] | (dist << 8),) if ncol == 7 else row)
    first, nchunks = ops.chunk_first(MULTI_SIZES)
    return ts, torch.tensor(rows, dtype=torch.int64).cuda(), torch.tensor(first, dtype=torch.int32).cuda(), nchunks


def dump(path):
    out = []                                   # (name, bytes)

    def record(case, tensors, before=None):
        for k, t in enumerate(tensors):
            if t is not None:
                out.append((f"{case}/{k}", raw(t)))
                if before is not None and before[k] != out[-1][1]:
                    raise SystemExit(f"{case}: tensor {k} changed although *skip was non-zero")

    def run(case, tensors, step_fn):
        for var in VARIATIONS:
            gen = torch.Generator().manual_seed(1234)
            ts = tensors(gen)
            kw = variation(var)
            flat = [t for group in ts for t in group]
            before = [None if t is None else raw(t) for t in flat] if var == "skip_set" else None
            for step in (1, 2, 3):
                step_fn(ts, step, kw)
            torch.cuda.synchronize()
            record(f"{case}/{var}", flat, before)

    # flat
    n = 2 * 4096 + 3
    for shadow in (False, True):
        def tensors(gen):
            return [(rnd(gen, n, 1.0), rnd(gen, n, 0.1), rnd(gen, n, 0.0), rnd(gen, n, 0.0),
                     torch.zeros(n, dtype=torch.bfloat16, device="cuda") if shadow else None)]
        run(f"flat/shadow{int(shadow)}", tensors,
            lambda ts, step, kw: ops.adamw_flat(*ts[0], 1e-3, 0.9, 0.999, 1e-8, 0.05, step, **kw))
    # flat groups: one call, and three ranges
    npad = (sum(SEG_SIZES) + 3) // 4 * 4
    ends, gids = segments(npad)
    seg_end, seg_group = torch.tensor(ends, dtype=torch.int64).cuda(), torch.tensor(gids, dtype=torch.int32).cuda()

    def seg_tensors(gen):
        return [(rnd(gen, npad, 1.0), rnd(gen, npad, 0.1), rnd(gen, npad, 0.0), rnd(gen, npad, 0.0),
                 torch.zeros(npad, dtype=torch.bfloat16, device="cuda"))]
    for name, cuts in (("whole", [0, npad]), ("ranges", [0, 5768, 9868, npad])):
        def step_fn(ts, step, kw):
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                ops.adamw_flat_groups(*(t[lo:hi] for t in ts[0]), lo, seg_end, seg_group, GROUPS3, step, **kw)
        run(f"flat_groups/{name}", seg_tensors, step_fn)
    # multi, 6 columns
    keep = []

    def multi6(gen):
        ts, table, first, nch = multi_case(gen, ["copy" if i % 2 else "none" for i in range(len(MULTI_SIZES))], None, 6)
        keep[:] = [table, first, nch]
        return ts
    run("multi6", multi6, lambda ts, step, kw: ops.adamw_multi(keep[0], keep[1], len(ts), keep[2], 1e-3, 0.9, 0.99, 1e-8, 0.05, step, **kw))
    # multi, 7 columns, every rotation of the image kinds
    for rot in range(len(KINDS)):
        def multi7(gen):
            kinds = [KINDS[(i + rot) % len(KINDS)] for i in range(len(MULTI_SIZES))]
            ts, table, first, nch = multi_case(gen, kinds, [i % 2 for i in range(len(MULTI_SIZES))], 7)
            keep[:] = [table, first, nch]
            return ts
        run(f"multi7/rot{rot}", multi7, lambda ts, step, kw: ops.adamw_multi_groups(keep[0], keep[1], len(ts), keep[2], GROUPS3[1:], step, **kw))
    # EMA
    gen = torch.Generator().manual_seed(99)
    pairs, entries = [], []
    for i, n in enumerate(MULTI_SIZES):
        off = 1 if i == UNALIGNED else 0
        s, p = rnd(gen, n, 1.0, off), rnd(gen, n, 1.0, off)
        pairs.append((s, p))
        entries += [s.data_ptr(), p.data_ptr(), n, 1 if i == 2 else 0]
    first, nch = ops.chunk_first(MULTI_SIZES)
    table, first = torch.tensor(entries, dtype=torch.int64).cuda(), torch.tensor(first, dtype=torch.int32).cuda()
    for omd in (1.0, 1 - 0.9, 1 - 0.9999):
        ops.ema_multi(table, first, len(pairs), nch, omd)
    torch.cuda.synchronize()
    record("ema", [t for pair in pairs for t in pair])

    with open(path, "wb") as f:
        head = json.dumps([(name, len(b)) for name, b in out]).encode()
        f.write(len(head).to_bytes(8, "little") + head)
        for _, b in out:
            f.write(b)
    print(f"{len(out)} tensors, {sum(len(b) for _, b in out)} bytes -> {path}   (library: {os.environ.get('MUSE_HIP_LIB', 'in-tree')})")


def load(path):
    with open(path, "rb") as f:
        head = json.loads(f.read(int.from_bytes(f.read(8), "little")))
        return [(name, f.read(n)) for name, n in head]


def compare(a, b):
    A, B = load(a), load(b)
    if [(n, len(x)) for n, x in A] != [(n, len(x)) for n, x in B]:
        raise SystemExit("the two dumps do not hold the same tensors")
    bad = 0
    for (name, x), (_, y) in zip(A, B):
        d = sum(1 for u, w in zip(x, y) if u != w) if x != y else 0
        if d:
            print(f"DIFFERENT {name}: {d} of {len(x)} bytes")
        bad += d
    print(f"{len(A)} tensors, {sum(len(x) for _, x in A)} bytes compared: {bad} differing bytes")
    sys.exit(1 if bad else 0)


def median_us(fn, warmup=5, launches=20):
    step = 0
    for _ in range(warmup):
        step += 1
        fn(step)
    torch.cuda.synchronize()
    events = []
    for _ in range(launches):
        step += 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(step)
        e1.record()
        events.append((e0, e1))
    torch.cuda.synchronize()
    return round(1000.0 * statistics.median(a.elapsed_time(b) for a, b in events), 2)


def time_lion():
    """lion_multi against adamw_multi over the parameter table of BASELINE config 4 (MaskGiTUViT, bf16 copies of every tensor), and
    lion_flat against adamw_flat over the flat buffer of the configs/imagenet.yaml transformer with its bf16 shadow: each pair in this
    one process, on the same p, g, m and images.  TB/s counts 30 (AdamW) / 22 (Lion) bytes per element."""
    import muse
    import weights as W
    dev_gen = torch.Generator(device="cuda").manual_seed(5)

    def normal(n, scale):
        return torch.empty(n, dtype=torch.float32, device="cuda").normal_(generator=dev_gen).mul_(scale)

    def pair(res, name, n, adamw, lion):
        # AdamW, Lion, AdamW, Lion: the two medians of each are reported so that the pair's own drift shows
        a = [median_us(adamw), None]
        li = [median_us(lion), None]
        a[1], li[1] = median_us(adamw), median_us(lion)
        res[name] = dict(elements=n, adamw_us=a, lion_us=li, adamw_tb_s=round(30.0 * n / min(a) / 1e6, 3), lion_tb_s=round(22.0 * n / min(li) / 1e6, 3),
                         lion_over_adamw=round(statistics.median(li) / statistics.median(a), 4))
    res = {"library": os.environ.get("MUSE_HIP_LIB", "in-tree")}
    with torch.device("meta"):
        sizes = [q.numel() for q in muse.MaskGiTUViT(**W.UVIT_CC12M).parameters()]
    rows, keep = [], []
    for sz in sizes:
        p, g, m, v = normal(sz, 0.02), normal(sz, 0.01), torch.zeros(sz, device="cuda"), torch.zeros(sz, device="cuda")
        sh = torch.zeros(sz, dtype=torch.bfloat16, device="cuda")
        keep.append((p, g, m, v, sh))
        rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr(), sz))
    first, nch = ops.chunk_first(sizes)
    first, table = torch.tensor(first, dtype=torch.int32).cuda(), torch.tensor(rows, dtype=torch.int64).cuda()
    res["multi_tensors"] = len(sizes)
    pair(res, "multi", sum(sizes),
         lambda step: ops.adamw_multi(table, first, len(sizes), nch, 1e-4, 0.9, 0.999, 1e-8, 0.01, step),
         lambda step: ops.lion_multi(table, first, len(sizes), nch, 1e-4, 0.9, 0.99, 0.01))
    del keep, rows, table
    model = muse.MaskGitTransformer(**W.TRANSFORMER_B).to("cuda")
    n = model.flat_params().numel()
    del model
    p, g, m, v = normal(n, 0.02), normal(n, 0.01), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    pair(res, "flat", n,
         lambda step: ops.adamw_flat(p, g, m, v, sh, 1e-4, 0.9, 0.999, 1e-8, 0.01, step),
         lambda step: ops.lion_flat(p, g, m, sh, 1e-4, 0.9, 0.99, 0.01))
    print(json.dumps(res))


def time_kernels():
    import muse
    import weights as W
    dev_gen = torch.Generator(device="cuda").manual_seed(5)

    def normal(n, scale):
        return torch.empty(n, dtype=torch.float32, device="cuda").normal_(generator=dev_gen).mul_(scale)

    res = {"library": os.environ.get("MUSE_HIP_LIB", "in-tree")}
    # the flat buffer of the configs/imagenet.yaml transformer, with its bf16 shadow; segments = its parameters, matrices decayed
    model = muse.MaskGitTransformer(**W.TRANSFORMER_B).to("cuda")
    n = model.flat_params().numel()
    ends, gids = [], []
    for q, o in zip(model._param_order(), model._offsets):
        k = 0 if q.ndim >= 2 else 1
        if gids and gids[-1] == k:
            ends[-1] = o + q.numel()
        else:
            ends.append(o + q.numel())
            gids.append(k)
    ends[-1] = n
    del model
    seg_end, seg_group = torch.tensor(ends, dtype=torch.int64).cuda(), torch.tensor(gids, dtype=torch.int32).cuda()
    p, g, m, v = normal(n, 0.02), normal(n, 0.01), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    res["flat_elements"], res["flat_segments"] = n, len(ends)
    res["flat_us"] = median_us(lambda step: ops.adamw_flat(p, g, m, v, sh, 1e-4, 0.9, 0.999, 1e-8, 0.01, step))
    res["flat_groups_us"] = median_us(lambda step: ops.adamw_flat_groups(p, g, m, v, sh, 0, seg_end, seg_group, GROUPS3[:2], step))
    del p, g, m, v, sh
    # a table of 400 tensors: 200 matrices of 1024 x 1024 with operand planes behind them, 200 vectors of 4099 elements without an image
    sizes = [1024 * 1024, 4099] * 200
    rows6, rows7, keep = [], [], []
    for i, sz in enumerate(sizes):
        p, g, m, v = normal(sz, 0.02), normal(sz, 0.01), torch.zeros(sz, device="cuda"), torch.zeros(sz, device="cuda")
        planes = torch.zeros(2 * sz, dtype=torch.bfloat16, device="cuda") if i % 2 == 0 else None
        keep.append((p, g, m, v, planes))
        row = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if planes is None else planes.data_ptr(), sz)
        rows6.append(row)
        rows7.append(row + ((i % 2) | ((sz if planes is not None else 0) << 8),))
    first, nch = ops.chunk_first(sizes)
    first = torch.tensor(first, dtype=torch.int32).cuda()
    t6, t7 = torch.tensor(rows6, dtype=torch.int64).cuda(), torch.tensor(rows7, dtype=torch.int64).cuda()
    res["multi_tensors"], res["multi_elements"] = len(sizes), sum(sizes)
    res["multi7_us"] = median_us(lambda step: ops.adamw_multi_groups(t7, first, len(sizes), nch, GROUPS3[:2], step))
    res["multi6_us"] = median_us(lambda step: ops.adamw_multi(t6, first, len(sizes), nch, 1e-4, 0.9, 0.999, 1e-8, 0.01, step))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="FILE")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--time-lion", action="store_true")
    ap.add_argument("--limit", type=float, default=240.0, help="seconds the run may take before the process is ended")
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.limit, exit=True)
    if args.compare:
        compare(*args.compare)
    elif args.dump:
        dump(args.dump)
    elif args.time:
        time_kernels()
    elif args.time_lion:
        time_lion()
    else:
        ap.error("one of --dump, --compare, --time, --time-lion")


if __name__ == "__main__":
    main()
