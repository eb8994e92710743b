"""The patch-slab convolution kernels of two builds of libmuse_hip.so, bit for bit and launch for launch (csrc/conv_dma.hip against the build
before it):

    MUSE_HIP_LIB=/path/to/libmuse_hip.so python scripts/conv_parent_ab.py --dump FILE    # every case below -> FILE (raw bytes of every output)
    python scripts/conv_parent_ab.py --compare A B                                       # demands A == B byte for byte (exit 1 otherwise)
    MUSE_HIP_LIB=... python scripts/conv_parent_ab.py --time                             # HIP events: 5 warm-up + 20 timed launches, median per case

One process per library (the library is chosen when muse is imported), and - because the library reads its MUSE_CONV_* switches once - one
child process per setting of them, started by --dump itself:
  launch     persistent = 0: conv_slab_kernel<false>, <true, false>, <true, true>
  persist    MUSE_CONV_PERSIST=1 MUSE_CONV_PERSIST_MIN=0 MUSE_CONV_PERSIST_GRID=3: conv_slab_persist_kernel<true, *> on three workgroups, which
             walk several tiles across image and column-tile changes
  slab2      MUSE_CONV_SLAB=2: conv_slab_persist_kernel<false>, grid min(tiles, CUs): the list below and the 2 CUs + 1 tiles shape of
             tests/test_gpu_conv_edges.py::test_slab_split2_more_tiles_than_cus, the one where its workgroups walk
Cases: (B, H, W) in (1, 16, 16) all-padding halo, (2, 32, 16) image change inside the walk, (1, 48, 48) interior patch; Cin in 64, 128, 320
(one and two chunk pairs, an odd chunk count; 320 > P_GSS_MAX_CIN keeps the fused forms on the launch-per-tile kernel); Cout in 4, 132, 256
(ragged tile, two column tiles); bias + residual + GroupNorm partials (32 groups, where Cout allows them) on, and all off; the forms split2
(planes in), gn_split2 and gn_split2_pool (f32 in, scale / shift).  Inputs are random normal f32 from a seeded CPU generator.  The output tensor
and the f64 partial slab are dumped as raw bytes.
--time runs the workload's own shapes, each with persistent 0 and 1 where the route exists.
The whole run is ended with a traceback if it exceeds --limit seconds."""
import argparse
import faulthandler
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))

SHAPES = [(1, 16, 16), (2, 32, 16), (1, 48, 48)]
CINS, COUTS = [64, 128, 320], [4, 132, 256]
FORMS = ("split2", "gn_split2", "gn_split2_pool")
CHILDREN = {
    "launch": dict(MUSE_CONV_PERSIST="0"),
    "persist": dict(MUSE_CONV_PERSIST="1", MUSE_CONV_PERSIST_MIN="0", MUSE_CONV_PERSIST_GRID="3"),
    "slab2": dict(MUSE_CONV_SLAB="2", MUSE_CONV_PERSIST="0"),
}
# (form, B, H, W, Cin, Cout) of the tokenizer at the benchmark's batch
TIME_SHAPES = [("gn_split2", 64, 256, 256, 128, 128), ("gn_split2_pool", 64, 256, 256, 128, 128), ("gn_split2", 64, 64, 64, 256, 256),
               ("gn_split2", 64, 16, 16, 512, 512), ("split2", 64, 128, 128, 128, 128)]


def raw(t):
    import torch
    return t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()


def tiles_shape(T):
    """(B, H, W) with B * (H / 16) * (W / 16) == T and the image as square as T's factors allow (tests/test_gpu_conv_edges.py)"""
    best = None
    for b in range(1, 9):
        if T % b:
            continue
        r = T // b
        th = max(d for d in range(1, int(r ** 0.5) + 1) if r % d == 0)
        cand = (r // th - th, b, th, r // th)
        best = cand if best is None or cand < best else best
    _, b, th, tw = best
    return b, 16 * th, 16 * tw


def operands(gen, form, B, H, W, Cin, Cout, extras):
    """-> the call's tensors on the device, drawn by `gen` (the dumps: a CPU generator; the timed shapes: one of the device)"""
    import torch
    from muse import ops

    def normal(*shape):
        return torch.randn(*shape, generator=gen, device=gen.device).cuda()
    x = normal(B, H, W, Cin) * 1.5
    w_hi, w_lo = ops.split_bf16(normal(Cout, 9 * Cin) * 0.05)
    scale = 1.0 + 0.25 * normal(B, Cin)
    shift = 0.25 * normal(B, Cin)
    bias = normal(Cout) if extras else None
    residual = normal(B, H, W, Cout) if extras else None
    o = dict(w_hi=w_hi, w_lo=w_lo, bias=bias, residual=residual, groups=32 if extras else 0)
    if form == "split2":
        o["x_hi"], o["x_lo"] = ops.split_bf16(x)
    else:
        o["x"], o["scale"], o["shift"] = x, scale, shift
    return o


def run(form, o, B, H, W, Cin, Cout):
    from muse import ops
    if form == "split2":
        return ops.conv2d_nhwc_split2(o["x_hi"], o["x_lo"], o["w_hi"], o["w_lo"], B, H, W, Cin, Cout, o["bias"], o["residual"], o["groups"])
    fn = ops.conv2d_nhwc_gn_split2 if form == "gn_split2" else ops.conv2d_nhwc_gn_split2_pool
    return fn(o["x"], o["scale"], o["shift"], o["w_hi"], o["w_lo"], B, H, W, Cin, Cout, o["bias"], o["residual"], o["groups"])


def write_dump(path, out):
    with open(path, "wb") as f:
        head = json.dumps([(name, len(b)) for name, b in out]).encode()
        f.write(len(head).to_bytes(8, "little") + head)
        for _, b in out:
            f.write(b)


def load(path):
    with open(path, "rb") as f:
        head = json.loads(f.read(int.from_bytes(f.read(8), "little")))
        return [(name, f.read(n)) for name, n in head]


def dump_child(name, path):
    """the cases of one setting of the library's switches (this process was started with them)"""
    import torch
    from muse import ops
    out = []
    forms = {"launch": FORMS, "persist": FORMS[1:], "slab2": FORMS[:1]}[name]
    cases = [(form, B, H, W, Cin, Cout) for form in forms for (B, H, W) in SHAPES for Cin in CINS for Cout in COUTS]
    if name == "slab2":
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        cases.append(("split2",) + tiles_shape(2 * ncu + 1) + (64, 8))
    for form, B, H, W, Cin, Cout in cases:
        for extras in (True, False):
            gen = torch.Generator().manual_seed(4321)
            o = operands(gen, form, B, H, W, Cin, Cout, extras)
            with ops.conv_persistent(name == "persist"):
                y = run(form, o, B, H, W, Cin, Cout)
            torch.cuda.synchronize()
            case = f"{name}/{form}/{B}x{H}x{W}/{Cin}->{Cout}/{'all' if extras else 'none'}"
            out.append((case + "/out", raw(y)))
            stats = getattr(y, "_gn_stats", None)
            if stats is not None:
                out.append((case + "/partials", raw(stats[0])))
    write_dump(path, out)


def dump(path, limit):
    out = []
    for name, env in CHILDREN.items():
        part = f"{path}.{name}"
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--dump", part, "--limit", str(limit)], check=True,
                       env=dict(os.environ, **env), timeout=limit)
        out += load(part)
        os.remove(part)
    write_dump(path, out)
    print(f"{len(out)} tensors, {sum(len(b) for _, b in out)} bytes -> {path}   (library: {os.environ.get('MUSE_HIP_LIB', 'in-tree')})")


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


def time_kernels(warmup=5, launches=20):
    import torch
    from muse import ops
    res = {"library": os.environ.get("MUSE_HIP_LIB", "in-tree")}
    for form, B, H, W, Cin, Cout in TIME_SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(7)
        o = operands(gen, form, B, H, W, Cin, Cout, True)
        for persistent in ((0,) if form == "split2" or Cin > 256 else (0, 1)):
            with ops.conv_persistent(bool(persistent)):
                for _ in range(warmup):
                    run(form, o, B, H, W, Cin, Cout)
                torch.cuda.synchronize()
                events = []
                for _ in range(launches):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(form, o, B, H, W, Cin, Cout)
                    e1.record()
                    events.append((e0, e1))
                torch.cuda.synchronize()
            res[f"{form}/{B}x{H}x{W}/{Cin}->{Cout}/persistent{persistent}_us"] = round(1000.0 * statistics.median(a.elapsed_time(b) for a, b in events), 2)
        del o
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="FILE")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--child", choices=sorted(CHILDREN), help=argparse.SUPPRESS)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds the run may take before the process is ended")
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.limit, exit=True)
    if args.compare:
        compare(*args.compare)
    elif args.dump and args.child:
        dump_child(args.child, args.dump)
    elif args.dump:
        dump(args.dump, args.limit)
    elif args.time:
        time_kernels()
    else:
        ap.error("one of --dump, --compare, --time")


if __name__ == "__main__":
    main()
