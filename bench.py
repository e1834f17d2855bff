"""Throughput benchmark of the MI355X inference path (contract: see the task's bench rules).

One step = one pass of the hot path over one batch of synthetic frames: mpe_match_batch
(featurise + GAT + clustering) followed by mpe_mlp3d_batch (MLP 3D), i.e. BASELINE.json
configs[1] ("Panoptic 5-view, 4-person; GATv2 match + MLP 3D, 1k-frame batch on 1 MI355X").
With --mode tri the 3D stage is the DLT triangulation path (configs[2]).

Launch.  `python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment starts N
rank processes ITSELF (fresh children; the parent makes no HIP call and does not import torch; RANK /
LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment) and relays rank 0's JSON line; under
torchrun (`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`) the ranks already exist
and are used; `--gpus` must equal WORLD_SIZE (a mismatch exits 3 before any GPU work).  One process per GPU, RCCL (`--backend nccl`) for the only exchange of the
path: one all-gather of the 3D poses per step.

Scaling modes.  Default (weak): every rank processes its own `--frames`-frame shard per step.
`--total-frames T` (strong, configs[3]: 100 000 frames of 5 views x 10 persons over 8 GPUs): the
T frames are cut into contiguous shards (distributed.shard_range), every rank runs its shard and
all ranks receive all T results (distributed.all_gather_results).

Plain run and --full.  A plain run (`bench.py --gpus 1 --steps N --warmup W`) does only what `value` needs: set-up,
W warm-up steps, ONE timed region of exactly N steps, the outputs of its last step if `--dump-outputs DIR` is given,
and the JSON line.  Everything else described below -- the further timed regions of the headline (value = their
median), io_inclusive, json_inclusive, dropin_loop, the MLP's accuracy modes, the kernel-level roofline pass, the
parity sample and the CPU baseline, the gather check after the timed region -- runs with `--full` only; in a plain
run those fields of the line are null.

--dump-outputs DIR.  After the timed region: what its last step returned, as a caller of the path receives it (with
N > 1 ranks: the gathered result, written by rank 0), in DIR/poses.npy ([frames, persons capacity, joints, 3]; float32
for the MLP path, float64 for DLT; slots past a frame's person count zeroed: they hold no result), DIR/n_persons.npy
and DIR/frame_index.npy (float64).  Beyond 64 MB, a fixed seeded sample of the frames (frame_index says which).  The
frames and weights are hash-generated, so the same arguments give the same inputs on every run.

What is timed.  `value` = whole-job frames/s with the packed 2D skeletons already resident in HBM
when the timed region starts and the poses left in HBM (barrier + synchronize on both sides, max
over ranks; the bench contract's definition -- "inputs already resident in HBM when the timed region
starts", a PCIe-inclusive rate is never `value`).  The figure SURVEY.md 8(d) words -- pinned host ->
poses in pinned host -- is the region `io_inclusive` and is repeated at the top level of the line as
`value_host_to_host` so that nobody has to dig for it; `value_json_cold` is the first pass over
wire-format JSON bytes.  The engine
runs in its default mode: two contexts (own workspace, same weights: Engine.sibling) take turns on the
steps, each on its own stream, so two whole steps are in flight and fill each other's launch tails
(`--contexts 2`, Engine.run_pipelined(contexts=2)).  `--contexts 1 --streams 2` = one context with the
matching stage of step i+1 beside the 3D stage of step i; `--contexts 1 --streams 1` = one stream.
Further timed regions, reported BESIDE `value`:
  io_inclusive    SURVEY.md §8(d) as worded: packed batch in pinned host memory -> one H2D copy ->
                  compute -> D2H of poses and person counts into pinned memory, double-buffered
  json_inclusive  SURVEY.md §8 f1: the reference's wire format (frame JSON bytes in host memory) ->
                  native packer -> H2D -> compute -> poses in pinned host memory (Engine.stream_json)

The JSON line also carries
  roofline      fp32-MFMA GEMM kernel: algorithmic FLOPs of its launches / their summed duration,
                measured with HIP events on the launch stream in a single-stream pass of
                `--profile-steps` steps after the timed region (with two streams the kernels of
                two steps overlap and a launch's duration means nothing); peak = 157.3 TFLOP/s
                fp32 matrix (MI355X_MICROARCH.md); `step` = GEMM FLOPs of a step / wall time of a
                step of the timed region (everything the step does, priced against the same
                peak); `hbm` = compulsory bytes of the path per second / 8 TB/s;
                `traffic` = fabric bytes per GEMM launch from the committed rocprofv3 PMC passes
  parity        a sample in the CAPTURE-VOLUME regime (hand-built matcher network + decoder MLP with
                dense hash noise: correct clusters, poses within a few metres, a meaningful MPJPE)
                through the HIP path and through the CPU oracle: clusters, max |3D difference| in mm
                and in ulps, each side's distance from the exactly evaluated network, MPJPE
  cpu_baseline  the CPU oracle (oracle/oracle_np.py, a port of the reference's algorithm on
                torch-CPU) timed on rank 0 on a bounded sample of the same frames.
"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = '3d_multi_pose_estimator_amd'

PEAK_FP32_MFMA_TFLOPS = 157.3
PEAK_BF16_MFMA_TFLOPS = 2500.0      # dense (MI355X_MICROARCH.md; the 5 PF headline figure includes 2:1 sparsity)
PEAK_HBM_TBS = 8.0
DUMP_BYTES = 64 * 10 ** 6 - 4096      # --dump-outputs: at most 64 MB in all (the .npy headers included)


def traffic_files():
    """profiles/rNN_pmc_traffic.json, newest round first (the record of THIS round when its profile pass has been committed)."""
    import glob
    import re
    found = []
    for path in glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_traffic.json')):
        m = re.match(r'r(\d+)_pmc_traffic\.json$', os.path.basename(path))
        if m:
            found.append((int(m.group(1)), os.path.basename(path)))
    return [name for _, name in sorted(found, reverse=True)]


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--full', action='store_true',
                    help='besides the headline: further timed regions, io / JSON / drop-in regions, accuracy modes, kernel-level '
                         'roofline, parity sample and CPU baseline (a plain run times --steps steps once and prints the line)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step returned (poses, person counts) to DIR/*.npy')
    ap.add_argument('--regions', type=int, default=None,
                    help='timed regions of --steps steps each; value = the median region (default: 1, with --full 3)')
    ap.add_argument('--frames', type=int, default=1000, help='frames per rank and step (weak scaling)')
    ap.add_argument('--total-frames', type=int, default=0,
                    help='strong scaling: this many frames per step in total, sharded over the ranks (configs[3]: 100000 with --persons 10)')
    ap.add_argument('--persons', type=int, default=4)
    ap.add_argument('--mode', choices=['mlp', 'tri'], default='mlp')
    ap.add_argument('--cpu-sample', type=int, default=40, help='frames of the CPU baseline / parity sample (0 = skip)')
    ap.add_argument('--fast-mlp', action='store_true', help='plain fp32 accumulation in the MLP GEMMs')
    ap.add_argument('--gat-acc', choices=['default', 'f32', 'f64'], default='default',
                    help='accumulation of the GAT GEMMs: one fp32 MFMA chain, or f64 running sums per 32-deep K stage')
    ap.add_argument('--gat-fp32-mfma', action='store_true',
                    help='GAT GEMMs of layers >= 1 on the fp32 MFMA (the default of rounds 1-3) instead of the split-bf16 form')
    ap.add_argument('--mlp-fp32-mfma', action='store_true',
                    help='MLP GEMMs on the fp32 MFMA with f64 running sums per K stage (the default of rounds 1-3) instead of the '
                         'split-bf16 form (same accuracy class, csrc/gemm_sb16.hip)')
    ap.add_argument('--bf16-mlp', action='store_true',
                    help='reduced precision (NOT the parity path): bf16 MFMA for the MLP GEMMs, configs[4] style')
    ap.add_argument('--reduced', action='store_true',
                    help='configs[4] precision (NOT the parity path): bf16 MFMA for the GAT and MLP GEMMs, fp16 '
                         'feature rows in the attention stage')
    ap.add_argument('--cfg4', action='store_true',
                    help='BASELINE configs[4] precision as worded (NOT the parity path): fp16 feature rows in the attention '
                         'stage (GAT GEMMs stay fp32) + bf16 MFMA for the MLP GEMMs')
    ap.add_argument('--preset', default='PANOPTIC', choices=['PANOPTIC', 'ARPLAB', 'RING23'],
                    help='camera rig; RING23 = the 23-view stress rig of BASELINE.json configs[4] (fp32 here)')
    ap.add_argument('--backend', default='nccl', help='torch.distributed backend (nccl = RCCL; gloo only to rehearse)')
    ap.add_argument('--streams', type=int, default=2, choices=[1, 2],
                    help='2 (default engine mode) = software pipeline across steps: matching of batch i+1 overlaps the 3D '
                         'stage of batch i on a second stream; 1 = everything on one stream')
    ap.add_argument('--contexts', type=int, default=2,
                    help='2 (default engine mode): two contexts (own workspace, same weights) take turns on the steps, one stream '
                         'each, so two whole steps are in flight; 1 = one context (--streams then says how its stages run)')
    ap.add_argument('--profile-steps', type=int, default=24,
                    help='single-stream steps after the timed region with HIP event pairs around the GEMM launches '
                         '(kernel-level roofline); 0 = skip')
    ap.add_argument('--json-steps', type=int, default=96,
                    help='batches of the json_inclusive region (wire-format JSON bytes -> poses in pinned host memory); 0 = skip')
    ap.add_argument('--dropin-frames', type=int, default=200,
                    help="frames of the dropin_loop region (the reference's one-frame-per-call loop over the drop-in mirrors); 0 = skip")
    ap.add_argument('--no-io', action='store_true', help='skip the second (pinned host -> poses in pinned host) timed region')
    ap.add_argument('--no-accuracy-modes', action='store_true',
                    help="skip the short timed regions of the MLP's maximum-accuracy (mode 4) and reference-exact (mode 5) forms (kernel "
                         'profiles of the default path)')
    ap.add_argument('--no-profile', action='store_true', help='no per-GEMM HIP events (roofline comes out null)')
    ap.add_argument('--profile-every', type=int, default=4,
                    help='HIP event pairs around the GEMM launches on every n-th step of the profile pass (the event packets '
                         'cost ~2 %% of a step when taken on every step)')
    ap.add_argument('--dry-run', action='store_true',
                    help='no GPU work: exercises launch, rendezvous, sharding and the all-gather with stand-in results '
                         '(CPU tests of the N > 1 path); prints no throughput')
    return ap.parse_args(argv)


# --------------------------------------------------------------------------------------------
# parent: start N ranks
# --------------------------------------------------------------------------------------------

def free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def visible_gpu_count():
    """Number of GPUs the rank processes will see, WITHOUT initialising HIP in this (parent)
    process: an explicit *_VISIBLE_DEVICES list if one is set, else the KFD topology in sysfs
    (a GPU node has simd_count > 0; CPU nodes have 0).  None if neither source exists -- the
    ranks then find out themselves (a rank without a device fails and takes the job down)."""
    for var in ('HIP_VISIBLE_DEVICES', 'ROCR_VISIBLE_DEVICES', 'CUDA_VISIBLE_DEVICES'):
        v = os.environ.get(var)
        if v is not None:
            return len([x for x in v.split(',') if x.strip() != ''])
    root = '/sys/class/kfd/kfd/topology/nodes'
    try:
        nodes = os.listdir(root)
    except OSError:
        return None
    n = 0
    for d in nodes:
        try:
            with open(os.path.join(root, d, 'properties')) as fh:
                for line in fh:
                    k, _, v = line.partition(' ')
                    if k == 'simd_count' and int(v) > 0:
                        n += 1
                        break
        except (OSError, ValueError):
            continue
    return n


def launch_ranks(args, count_fn=visible_gpu_count, popen=subprocess.Popen):
    """Parent of `python bench.py --gpus N`: N fresh rank processes, never a re-exec or fork of a
    process that has touched the GPU -- this one makes NO HIP call and never loads the torch module
    (the device count comes from the environment / sysfs, visible_gpu_count).  Rank 0 inherits
    stdout, so its JSON line is this command's output.  All children are polled together: the
    first rank that exits non-zero ends the job (its siblings would otherwise sit in the
    rendezvous or in the all-gather until their own timeout)."""
    n = args.gpus
    if not args.dry_run and args.backend == 'nccl':
        have = count_fn()
        if have is not None and have < n:
            print('bench.py: --gpus %d requested but %d GPU(s) visible' % (n, have), file=sys.stderr)
            return 2
    env = dict(os.environ)
    env.update({'WORLD_SIZE': str(n), 'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(free_port()),
                'HSA_ENABLE_IPC_MODE_LEGACY': '0', 'MPE_BENCH_SPAWNED': '1'})
    procs = []
    for r in range(n):
        e = dict(env)
        e['RANK'] = e['LOCAL_RANK'] = str(r)
        procs.append(popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=e,
                           stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    deadline = time.time() + float(os.environ.get('MPE_BENCH_RANK_TIMEOUT', '3000'))
    live = list(procs)
    try:
        while live and not rc:
            for p in list(live):
                code = p.poll()
                if code is None:
                    continue
                live.remove(p)
                if code:
                    rc = code
                    break
            if live and not rc:
                if time.time() > deadline:
                    rc = 124
                    break
                time.sleep(0.05)
    finally:
        for p in procs:                            # exact PIDs of our own children only
            if p.poll() is None:
                p.kill()
        for p in procs:
            try:
                p.wait(timeout=10)
            except Exception:
                pass
    if rc:
        print('bench.py: a rank exited with code %d; the remaining ranks were stopped' % rc, file=sys.stderr)
    return rc


# --------------------------------------------------------------------------------------------
# one rank
# --------------------------------------------------------------------------------------------

def run_rank(args):
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')      # before HIP initialises: one hardware queue per stream of the pipelines (lib.py)
    import numpy as np
    import torch
    import torch.distributed as dist

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if args.gpus != world and not os.environ.get('MPE_BENCH_FORCE_DIST'):
        # one contract: the ranks that exist ARE the job, and --gpus must say so (the driver always passes the same number to the
        # launcher and to bench.py).  A mismatch ends here, before any GPU work, instead of after a full step in the self-check.
        if rank == 0:
            print('bench.py: --gpus %d but WORLD_SIZE=%d: start as many ranks as --gpus names (python bench.py --gpus N spawns them itself; '
                  'under torchrun pass --nproc-per-node N and --gpus N)' % (args.gpus, world), file=sys.stderr)
        return 3
    # MPE_BENCH_FORCE_DIST=1: initialise the process group even at world size 1 (rehearses the RCCL
    # init / barrier / all-gather path on a one-GPU box)
    distributed = world > 1 or bool(os.environ.get('MPE_BENCH_FORCE_DIST'))
    use_gpu = not args.dry_run
    if distributed:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        if args.backend == 'nccl' and use_gpu:
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', local_rank))
        else:
            dist.init_process_group('gloo' if not use_gpu else args.backend, rank=rank, world_size=world)
    dmod = importlib.import_module(PKG + '.distributed')

    # ---- workload ---------------------------------------------------------------------------
    strong = args.total_frames > 0
    if strong:
        lo, hi, per = dmod.shard_range(args.total_frames, rank, world)
        B, cap, total = hi - lo, per, args.total_frames
    else:
        B = cap = args.frames
        lo, total = rank * B, B * world

    if args.dry_run:
        return dry_run(args, dist, dmod, world, rank, B, cap, total, strong)

    device = torch.device('cuda', local_rank % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(device)
    syn = importlib.import_module(PKG + '.synthetic')
    cal = importlib.import_module(PKG + '.calibration')
    par = importlib.import_module(PKG + '.parameters')
    pipeline = importlib.import_module(PKG + '.pipeline')
    packing = importlib.import_module(PKG + '.packing')
    params = par.select(args.preset)
    calib = cal.Calibration(params, syn.ring_transform_manager(params) if args.preset == 'RING23' else None)
    V, J = len(params.used_cameras_skeleton_matching), len(params.joint_list)
    nf = 2 + V * J * 10
    # logit shift chosen so that nearly every pair clears the 0.5 threshold: the greedy
    # clustering then assigns every skeleton, i.e. `persons` people per frame reach the MLP.
    gat_sd = syn.gat_state_dict(7, nf, logit_gain=25.0, logit_shift=0.698 + 0.25)
    prm = syn.gat_params(nf)
    in_dim = len(params.cameras) * J * params.numbers_per_joint
    mlp_sd = syn.mlp_state_dict(11, in_dim)

    spec = syn.FrameSpec(persons=args.persons)
    uniq = max(1, min(B, 250))                 # distinct frames per rank (frame index = global index)
    frames, wire = [], []
    for i in range(uniq):
        f, _ = syn.make_frame(calib, lo + i, spec)
        wire.append(f)                              # wire format: [json string, timestamp, 'no_image', bodies_3D] per camera
        frames.append({c: [f[c][0], f[c][1]] for c in f})
    frames = [frames[i % uniq] for i in range(B)]

    eng = pipeline.Engine(params, calib, max_frames=max(cap, 1), max_persons_per_camera=args.persons, device=str(device))
    eng.load_gat(gat_sd, prm)
    eng.load_mlp(mlp_sd)
    if args.gat_acc != 'default':
        eng.set_precision(args.gat_acc == 'f64', True)
    if args.fast_mlp:
        eng.set_precision(args.gat_acc == 'f64', False)
    if args.mlp_fp32_mfma or args.gat_fp32_mfma:
        eng.set_precision(args.gat_acc == 'f64', not args.fast_mlp, mlp_split=False if args.mlp_fp32_mfma else None,
                          gat_split=False if args.gat_fp32_mfma else None)
    if args.bf16_mlp:
        eng.set_precision(False, False, mlp_bf16=True)
    if args.reduced:
        eng.set_precision(False, False, mlp_bf16=True, gat_reduced=True)
    if args.cfg4:
        eng.set_precision(False, False, mlp_bf16=True, attn_fp16=True)
    pb = eng.pack(frames)
    eng.check_capacity(pb)
    db = eng.to_device(pb)
    torch.cuda.synchronize(device)
    if os.environ.get('MPE_BENCH_JSON_EARLY'):          # diagnostics: the JSON pipeline's streams and buffers made before any other stream
        list(eng.stream_json(json.dumps(wire[:2]).encode(), chunk_frames=B, mode=args.mode))
        torch.cuda.synchronize(device)

    K = max(1, args.contexts)
    engs = eng.contexts(K)              # K > 1: further contexts with the same weights and precision mode (Engine.sibling)
    ctx_streams = [torch.cuda.Stream(device) for _ in range(K)] if K > 1 else []
    s_match = torch.cuda.Stream(device) if (K == 1 and args.streams == 2) else None
    s_3d = torch.cuda.Stream(device) if (K == 1 and args.streams == 2) else None
    keep = []          # tensors produced on one stream and consumed on another stay referenced
    step_no = [0]

    def stage3d(batch, persons, n_persons, e=None):
        e = e or eng
        if args.mode == 'mlp':
            return e.mlp3d(batch, persons, n_persons)[0]
        return e.triangulate(batch, persons, n_persons)[0]

    def gather(poses, n_persons):
        """The path's only exchange: every rank receives the poses of all shards."""
        if not distributed:
            return poses, n_persons
        return dmod.all_gather_results(dmod.pad_to(poses, cap), dmod.pad_to(n_persons, cap), cap * world)

    def step_single():
        _, persons, n_persons = eng.match(db, want_scores=False)
        poses = stage3d(db, persons, n_persons)
        gather(poses, n_persons)
        return poses, n_persons

    def step():
        if K > 1:
            # the batch is read-only input: both contexts work from the same resident arrays, each in its own workspace
            k = step_no[0] % K
            step_no[0] += 1
            with torch.cuda.stream(ctx_streams[k]):
                _, persons, n_persons = engs[k].match(db, want_scores=False)
                poses = stage3d(db, persons, n_persons, engs[k])
                gather(poses, n_persons)
            keep.append((persons, n_persons, poses))
            if len(keep) > 2 * K:
                keep.pop(0)
            return poses, n_persons
        if args.streams != 2:
            return step_single()
        # the two stages use disjoint workspace, so matching of the next step may run
        # while the 3D stage of this one is still in flight
        with torch.cuda.stream(s_match):
            _, persons, n_persons = eng.match(db, want_scores=False)
            ev = torch.cuda.Event()
            ev.record(s_match)
        with torch.cuda.stream(s_3d):
            s_3d.wait_event(ev)
            poses = stage3d(db, persons, n_persons)
        for t_ in (persons, n_persons):
            t_.record_stream(s_3d)
        keep.append((persons, n_persons, poses))
        if len(keep) > 4:
            keep.pop(0)
        if not distributed:
            return poses, n_persons
        torch.cuda.current_stream(device).wait_stream(s_3d)
        gather(poses, n_persons)
        return poses, n_persons

    def timed(fn, steps):
        torch.cuda.synchronize(device)
        if distributed:
            dist.barrier()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        out = None
        for i in range(steps):
            out = fn(i)
        torch.cuda.synchronize(device)
        if distributed:
            dist.barrier()
        dt = time.perf_counter() - t0
        if distributed:
            t = torch.tensor([dt], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt, out

    for _ in range(K):           # initialisation (workspace, LDS attributes, communicator) of every context: not a warmup step
        step()
    torch.cuda.synchronize(device)
    for e in engs:
        e.sync_status()
    if distributed:
        # Before anything is timed: the process group has the size the command asked for, and one exchange puts every rank's own
        # shard, bit for bit, at its place in what it received.  A job that fails either check ends here with a non-zero code.
        ok_ws = dist.get_world_size() == args.gpus or bool(os.environ.get('MPE_BENCH_FORCE_DIST'))
        p0, n0 = step_single()
        torch.cuda.synchronize(device)
        ok_g = check_gather(torch, dist, gather, p0, n0, rank, cap, B, device)
        if not (ok_ws and ok_g):
            if rank == 0:
                print('bench.py: distributed self-check failed before the timed region: world size %d (asked for %d), gathered == local: %s'
                      % (dist.get_world_size(), args.gpus, ok_g), file=sys.stderr)
            dist.destroy_process_group()
            return 3
    for _ in range(args.warmup):
        step()

    # The headline region is timed `--regions` times in this process (a plain run: once; --full: 3), each EXACTLY --steps steps
    # between barrier + synchronize; `value` is the MEDIAN region, value_min / value_max the slowest / fastest: one region of 20
    # steps is 75 ms, and a single sample of it moved by 2 % between boards and runs without any code change (BENCH_r04 / r05).
    n_regions = args.regions if args.regions is not None else (3 if args.full else 1)
    regions = []
    for _ in range(max(1, n_regions)):
        dt_r, (poses, n_persons) = timed(lambda i: step(), args.steps)
        regions.append(dt_r)
    elapsed = sorted(regions)[len(regions) // 2]

    if args.dump_outputs:                    # the last timed step's results (timed() ended with a device synchronize)
        dump_outputs(args.dump_outputs, np, torch, dmod, gather, poses, n_persons, distributed, rank, world, cap, total, strong)

    # the exchange once more, checked: every rank finds its own shard, bit for bit, at its place in what it received
    gathered_ok = None
    if distributed and args.full:
        for s_ in [s_match, s_3d] + ctx_streams:
            if s_ is not None:
                torch.cuda.current_stream(device).wait_stream(s_)
        gathered_ok = check_gather(torch, dist, gather, poses, n_persons, rank, cap, B, device)

    # ---- kernel-level pass: one stream, HIP event pairs around the GEMM launches of every n-th step ----
    prof = None
    if args.full and not args.no_profile and args.profile_steps > 0:
        every = max(1, args.profile_every)
        for s_ in [s_match, s_3d] + ctx_streams:
            if s_ is not None:
                torch.cuda.current_stream(device).wait_stream(s_)
        for _ in range(3):
            step_single()
        eng.profile(True)
        eng.profile(False)

        def prof_step(i):
            eng.profile(i % every == 0, resume=True)
            return step_single()
        single_dt, _ = timed(prof_step, args.profile_steps)
        prof = eng.profile_read()
        eng.profile(False)
        prof['sampled_steps'] = len(range(0, args.profile_steps, every))
        prof['single_stream_ms_per_step'] = 1e3 * single_dt / args.profile_steps

    # ---- the MLP's maximum-accuracy mode (f64 flush per K stage) beside the default: same region, same engine mode, fewer steps ----
    max_acc = None
    plain_parity_path = args.mode == 'mlp' and not (args.reduced or args.cfg4 or args.bf16_mlp or args.fast_mlp or args.mlp_fp32_mfma)
    if args.full and plain_parity_path and not distributed and args.steps >= 10 and not args.no_accuracy_modes:
        for s_ in [s_match, s_3d] + ctx_streams:
            if s_ is not None:
                torch.cuda.current_stream(device).wait_stream(s_)
        eng.set_precision(args.gat_acc == 'f64', True, gat_split=False if args.gat_fp32_mfma else None, mlp_max_accuracy=True)
        for _ in range(max(4, 2 * K)):
            step()
        n_ma = max(10, args.steps // 4)
        dt_ma, _ = timed(lambda i: step(), n_ma)
        eng.set_precision(args.gat_acc == 'f64', True, gat_split=False if args.gat_fp32_mfma else None)
        for _ in range(2 * K):
            step()
        torch.cuda.synchronize(device)
        max_acc = {'value': total * n_ma / dt_ma, 'unit': 'frames/s', 'ms_per_step': 1e3 * dt_ma / n_ma, 'steps': n_ma,
                   'what': 'the timed region of `value` with the MLP in its maximum-accuracy mode (mpe_set_precision MLP 4: f64 flush after '
                           'every 32-deep K stage instead of every second one)'}
        # ... and in its reference-exact mode (MLP 5: exact products, f64 accumulation on the f64 matrix pipe)
        eng.set_precision(args.gat_acc == 'f64', True, gat_split=False if args.gat_fp32_mfma else None, mlp_f64=True)
        for _ in range(max(4, 2 * K)):
            step()
        n_fx = max(6, args.steps // 16)
        dt_fx, _ = timed(lambda i: step(), n_fx)
        eng.set_precision(args.gat_acc == 'f64', True, gat_split=False if args.gat_fp32_mfma else None)
        for _ in range(2 * K):
            step()
        torch.cuda.synchronize(device)
        max_acc['f64'] = {'value': total * n_fx / dt_fx, 'unit': 'frames/s', 'ms_per_step': 1e3 * dt_fx / n_fx, 'steps': n_fx}

    # ---- contract form: pinned host -> H2D -> compute -> D2H into pinned host, double-buffered ----
    io = None
    if args.full and not args.no_io:
        io = io_inclusive(args, torch, dist, packing, engs, pb, device, stage3d, gather, timed, distributed, total)
    jsn = None
    if args.full and (not args.no_io or os.environ.get('MPE_BENCH_JSON_WITHOUT_IO')) and args.json_steps > 0 and not distributed:
        jsn = json_inclusive(args, torch, eng, wire, B, uniq, K)

    # ---- the reference's own call pattern: ONE frame per call through the drop-in mirrors (metrics_from_model.py:178-294) ----
    dropin = None
    if args.full and args.dropin_frames > 0 and not distributed and args.preset == 'PANOPTIC' and args.mode == 'mlp' and not (args.reduced or args.cfg4 or args.bf16_mlp):
        loop = importlib.import_module(PKG + '.harness.dropin_loop')
        model_, mlp_ = loop.build_models(gat_sd, prm, mlp_sd)
        n_dl = args.dropin_frames
        # three passes over the same frames, the one with the median time inside the mirrors reported (the loop is host-bound: a single
        # pass moves by +-10 % with whatever else the host is doing), all three kept beside it
        passes = []
        for _ in range(3):
            r_ = loop.run([wire[i % uniq] for i in range(n_dl + 10)], model_, mlp_, warmup=10, device=device)
            r_.pop('last', None)
            passes.append(r_)
        res = sorted(passes, key=lambda r_: r_['inside_mirrors_ms'])[1]
        res['inside_mirrors_ms_passes'] = [round(r_['inside_mirrors_ms'], 4) for r_ in passes]
        res['ms_per_frame_passes'] = [round(r_['ms_per_frame'], 4) for r_ in passes]
        res['what'] = ("the loop body of the reference's test/metrics_from_model.py:178-294, one frame per call, over the package's "
                       'mirrors of its symbols (INTEGRATION.md section 2), timed with the reference\'s own two timers; '
                       'reference_readme_ms = what the reference README quotes for its own path on its authors\' GPU')
        dropin = res

    persons_per_frame = float(n_persons.float().mean().item()) if B else 0.0
    value = total * args.steps / elapsed
    reduced = args.reduced or args.bf16_mlp or args.cfg4
    out = {
        'metric': 'frames/sec (5-view Panoptic, 4 persons) at 1/2/4/8 GPUs; MPJPE vs ref',
        'value': value, 'unit': 'frames/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'full': args.full,
        'ms_per_step': 1e3 * elapsed / args.steps, 'higher_is_better': True, 'scaling': 'strong' if strong else 'weak',
        'value_min': total * args.steps / max(regions), 'value_max': total * args.steps / min(regions),
        'timed_regions': {'n': len(regions), 'steps_each': args.steps, 'ms_per_step': [1e3 * r / args.steps for r in regions],
                          'value_is': 'the median region'},
        'vs_baseline': None,
        'dtype': 'bf16 GEMMs / f16 attention rows' if args.reduced else 'f32 GAT GEMMs / f16 attention rows / bf16 MLP' if args.cfg4
                 else ('bf16 (MLP) / f32' if args.bf16_mlp else 'f32'),
        'data': 'synthetic',
        'config': {'workload': ('%s: %d-view x %d-person, GAT match + %s, %s'
                                % ('c2 Panoptic' if args.preset == 'PANOPTIC' else args.preset, V, args.persons,
                                   'MLP 3D' if args.mode == 'mlp' else 'DLT triangulation',
                                   ('%d frames per step sharded over %d GPU(s)' % (total, world)) if strong
                                   else '%d-frame batch per GPU' % B)),
                   'frames_per_step_per_gpu': B, 'frames_per_step_total': total,
                   'heads_per_batch': pb.n_heads, 'edge_nodes_per_batch': pb.n_edge_nodes,
                   'persons_found_per_frame': persons_per_frame, 'parallelism': 'frame-shard x%d' % world,
                   'world_size_seen': dist.get_world_size() if distributed else 1,
                   'gathered_equal_local': gathered_ok,
                   'backend': (args.backend + (' (RCCL)' if args.backend == 'nccl' else '')) if distributed else None,
                   'launcher': 'bench.py spawn' if os.environ.get('MPE_BENCH_SPAWNED') else ('torchrun' if distributed else 'single'),
                   'inputs': 'value: packed 2D skeletons resident in HBM, poses left in HBM (bench contract); '
                             'io_inclusive: pinned host -> poses in pinned host (SURVEY 8(d) as worded); '
                             'json_inclusive: wire-format JSON bytes -> poses in pinned host (SURVEY 8 f1)',
                   'contexts': K, 'streams': args.streams if K == 1 else 1,
                   'engine_mode': ('%d contexts (own workspace, same weights) taking turns on the steps, one stream each: %d steps in '
                                   'flight (default)' % (K, K)) if K > 1
                                  else ('one context, matching of step i+1 beside the 3D stage of step i on two streams' if args.streams == 2
                                        else 'one context, one stream'),
                   'mlp_accumulate': 'bf16 mfma (reduced precision)' if reduced else ('f32' if args.fast_mlp else 'f32 mfma + f64 running sums per K stage' if args.mlp_fp32_mfma
                                      else 'fp32 operands as three bf16 planes, six products on the bf16 mfma, f32 accumulators + f64 running sums every second K stage (fp32-accurate)'),
                   'gemm_arithmetic': ('reduced precision' if reduced else
                                       'fp32 in / fp32 out everywhere; GAT layers 1-4: %s; GAT layer 0 (head rows): fc1 per camera block (K = 180) on the fp32 MFMA, fc2 (K = 902) %s; MLP: see mlp_accumulate'
                                       % (('fp32 MFMA chain', 'on the fp32 MFMA with f64 running sums per K stage') if args.gat_fp32_mfma else
                                          ('fp32 operands as three bf16 planes, six products on the bf16 MFMA, fp32 accumulators (fp32-accurate)',
                                           'in the same split form with f64 running sums every second K stage'))),
                   'weights': 'deterministic hash init (no checkpoint offline)'},
        'value_resident': value,
        'value_host_to_host': io['value'] if io else None,
        'value_json_cold': jsn['value'] if jsn else None,
        'value_definitions': 'value = value_resident: packed input resident in HBM, poses left in HBM (the bench contract: "inputs already resident '
                             'in HBM when the timed region starts; a PCIe-inclusive rate is never value"); value_host_to_host = io_inclusive.value: '
                             'SURVEY 8(d) as worded, compact 2D keypoints in pinned host memory -> poses in pinned host memory (and gathered '
                             'when world > 1); value_json_cold = json_inclusive.value: wire-format JSON bytes read ONCE -> poses in pinned host memory',
        'io_inclusive': io,
        'json_inclusive': jsn,
        'dropin_loop': dropin,
    }
    if rank == 0:
        out['roofline'] = roofline(args, prof, elapsed, total, world, V, J, args.persons, reduced)
        # the CPU baseline and the parity sample are taken on rank 0 at N = 1 only, with --full
        base, par_ = (None, None) if world > 1 or not args.full else cpu_baseline_and_parity(args, np, torch, calib, params, lo, device)
        out['cpu_baseline'] = base
        if par_ is not None and max_acc is not None and par_.get('mlp_max_accuracy') is not None:
            par_['mlp_max_accuracy'].update({'frames_per_s': max_acc['value'], 'frames_per_s_default_mode': value,
                                             'ms_per_step': max_acc['ms_per_step'], 'timed': max_acc['what']})
            par_['mlp_f64_exact'].update({'frames_per_s': max_acc['f64']['value'], 'frames_per_s_default_mode': value,
                                          'ms_per_step': max_acc['f64']['ms_per_step']})
        out['parity'] = par_
        print(json.dumps(out), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()
    eng.close()
    return 0


def check_gather(torch, dist, gather, poses, n_persons, rank, cap, B, device):
    """One exchange, checked on every rank: its own shard sits, bit for bit, at its place in what it received (MIN over ranks)."""
    gp, gn = gather(poses, n_persons)
    mine = slice(rank * cap, rank * cap + B)
    ok = bool(torch.equal(gn[mine], n_persons[:B]))
    if ok and B:
        live = torch.arange(poses.shape[1], device=device)[None, :] < n_persons[:B, None].to(torch.int64)
        bits = torch.int32 if poses.dtype == torch.float32 else torch.int64          # NaN joints (DLT) compare as bits
        ok = bool(torch.equal(gp[mine][live].contiguous().view(bits), poses[:B][live].contiguous().view(bits)))
    t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(t.item())


def dump_outputs(out_dir, np, torch, dmod, gather, poses, n_persons, distributed, rank, world, cap, total, strong):
    """--dump-outputs: the poses and person counts of the last timed step as a caller receives them.  With N > 1 ranks
    every rank takes part in one more all-gather and rank 0 writes the frames of all shards, in global frame order.
    Slots past a frame's person count are zeroed (torch.empty: they hold no result); beyond DUMP_BYTES a fixed seeded
    sample of the frames is written, frame_index says which."""
    if distributed:
        gp, gn = gather(poses, n_persons)
        rows = []
        for r in range(world):
            r_lo, r_hi, _ = dmod.shard_range(total, r, world) if strong else (r * cap, (r + 1) * cap, cap)
            rows.append(torch.arange(r * cap, r * cap + (r_hi - r_lo), device=gp.device))
        rows = torch.cat(rows)
        poses, n_persons = gp[rows], gn[rows]
    if rank != 0:
        return
    p = poses.cpu().numpy()
    n = n_persons.cpu().numpy().astype(np.int64)
    live = np.arange(p.shape[1])[None, :] < n[:, None]
    p = np.where(live[:, :, None, None], p, np.zeros((), p.dtype)).astype(np.float64 if p.dtype == np.float64 else np.float32)
    idx = np.arange(p.shape[0])
    per_frame = p[:1].nbytes + 2 * 8
    if len(idx) * per_frame > DUMP_BYTES:
        idx = np.sort(np.random.default_rng(0).choice(len(idx), DUMP_BYTES // per_frame, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, 'poses.npy'), np.ascontiguousarray(p[idx]))
    np.save(os.path.join(out_dir, 'n_persons.npy'), n[idx].astype(np.float64))
    np.save(os.path.join(out_dir, 'frame_index.npy'), idx.astype(np.float64))


def io_inclusive(args, torch, dist, packing, engs, pb, device, stage3d, gather, timed, distributed, total):
    """SURVEY.md §8(d) metric as written: from compact 2D keypoints in host pinned memory to 3D
    poses back in host pinned memory.  K + 2 buffer sets; the H2D of step i+1 and the D2H of step
    i-1 run on two copy streams while step i (and, with K contexts, step i-1) computes."""
    pinned = packing.BatchArena(pb, 'pinned').fill(pb)
    K = len(engs)
    # Buffer sets: K steps computing + the one uploaded ahead + the one whose results are leaving.  The copy engines serve
    # H2D and D2H requests in ONE order: a D2H queued behind kernels that are still running holds up every upload queued
    # after it.  With K contexts the upload of step i must not wait for step i-1's results (step i-1 is still computing when
    # step i wants to start), so uploads run one step AHEAD and the D2H of step i-1 is queued after the launch of step i.
    NS = K + 2
    sets = []
    for _ in range(NS):
        arena = packing.BatchArena(pb, device)
        sets.append({'db': packing.DeviceBatch(pb, device, arena=arena), 'h2d': torch.cuda.Event(),
                     'done': torch.cuda.Event(), 'd2h': torch.cuda.Event(), 'out': None, 'host': None, 'used': False, 'sent': False})
    copy_s = torch.cuda.Stream(device)              # H2D of the batches
    back_s = torch.cuda.Stream(device)              # D2H of the results
    comp_s = torch.cuda.current_stream(device)
    # engine mode as in the main region: step g on context g % K (one stream each); with one context and --streams 2 the
    # matching stage and the 3D stage run on their own streams
    two = K == 1 and args.streams == 2 and not distributed
    lanes = []
    for k in range(K):
        if K > 1:
            st = torch.cuda.Stream(device)
            lanes.append((st, st))
        elif two:
            lanes.append((torch.cuda.Stream(device), torch.cuda.Stream(device)))
        else:
            lanes.append((comp_s, comp_s))
    state = {'g': 0, 'uploaded': 0, 'pending': None}

    def upload(g):
        b = sets[g % NS]
        with torch.cuda.stream(copy_s):
            if b['used']:
                copy_s.wait_event(b['done'])            # the batch buffer is free once step g - NS has computed
            b['db'].upload(pinned)
            b['h2d'].record(copy_s)

    def results_out(g):
        b = sets[g % NS]
        poses, n_persons, _ = b['out']
        with torch.cuda.stream(back_s):
            back_s.wait_event(b['done'])
            b['host'][0].copy_(poses, non_blocking=True)
            b['host'][1].copy_(n_persons, non_blocking=True)
            b['d2h'].record(back_s)
        b['sent'] = True

    def step(i, last=False):
        g = state['g']
        state['g'] += 1
        while state['uploaded'] <= g + 1:               # this step's batch (first call) and the next one
            upload(state['uploaded'])
            state['uploaded'] += 1
        b = sets[g % NS]
        eng = engs[g % K]
        m_s, d_s = lanes[g % K]
        m_s.wait_event(b['h2d'])
        if b['sent']:
            d_s.wait_event(b['d2h'])                    # step g - NS's results have left the output tensors
        with torch.cuda.stream(m_s):
            _, persons, n_persons = eng.match(b['db'], want_scores=False)
            ev = torch.cuda.Event()
            ev.record(m_s)
        with torch.cuda.stream(d_s):
            if d_s is not m_s:
                d_s.wait_event(ev)
            poses = stage3d(b['db'], persons, n_persons, eng)
            poses, n_persons = gather(poses, n_persons)
            b['done'].record(d_s)
        b['used'] = True
        for t_ in (persons, n_persons, poses):
            t_.record_stream(d_s)
            t_.record_stream(back_s)
        if b['host'] is None:
            b['host'] = (torch.empty(poses.shape, dtype=poses.dtype).pin_memory(),
                         torch.empty(n_persons.shape, dtype=n_persons.dtype).pin_memory())
        b['out'] = (poses, n_persons, persons)          # keep the tensors alive until their D2H is done
        if state['pending'] is not None:
            results_out(state['pending'])               # step g-1: behind this step's (and the next step's) upload in the copy queue
        state['pending'] = g
        if last:                                        # the region ends with every result in host memory
            results_out(g)
            state['pending'] = None
        return poses, n_persons

    for i in range(max(2, args.warmup)):
        step(i)
    dt, _ = timed(lambda i: step(i, i == args.steps - 1), args.steps)
    for s_ in {x for lane in lanes for x in lane} | {back_s, copy_s}:
        if s_ is not comp_s:
            comp_s.wait_stream(s_)
    return {'value': total * args.steps / dt, 'unit': 'frames/s', 'ms_per_step': 1e3 * dt / args.steps,
            'h2d_bytes_per_step': int(pinned.nbytes),
            'd2h_bytes_per_step': int(sum(t.numel() * t.element_size() for t in sets[0]['host'])),
            'what': 'packed batch in pinned host memory -> one H2D copy -> match + 3D stage -> D2H of poses and '
                    'n_persons into pinned host memory; %d buffer sets, uploads one step ahead, H2D and D2H on their own streams' % NS}


def roofline(args, prof, elapsed, total, world, V, J, persons, reduced):
    if prof is None:
        return None
    gemm_s = prof['gemm_ms'] * 1e-3
    achieved = prof['gemm_flop'] / gemm_s / 1e12 if gemm_s > 0 else 0.0
    traffic, src = pmc_traffic()
    # compulsory HBM bytes of the path per frame: compact input H*J*4 floats + H
    # camera ids, output P*54*4 + H*4, weights once per batch per GPU
    H = V * persons
    in_b = H * J * 4 * 4 + H * 4
    out_b = persons * J * 3 * 4 + H * 4
    nf = 2 + V * J * 10
    syn = importlib.import_module(PKG + '.synthetic')
    w_b = 4 * (sum(d * d + d + d * h * o + h * o + 2 * h * o for d, h, o in syn.gat_layer_dims(nf))
               + sum(i * o + o for i, o in syn.mlp_layer_dims(V * J * 14)))
    frames_per_gpu_step = total / world
    bytes_per_frame = in_b + out_b + w_b / max(1.0, frames_per_gpu_step)
    per_gpu_fps = total * args.steps / elapsed / world
    hbm_tbs = per_gpu_fps * bytes_per_frame / 1e12
    sampled = max(1, prof.get('sampled_steps', 1))
    split_flop, split_ms, split_n = prof.get('split_flop', 0.0), prof.get('split_ms', 0.0), prof.get('split_launches', 0)
    bf_flop, bf_ms, bf_n = prof.get('bf16_flop', 0.0), prof.get('bf16_ms', 0.0), prof.get('bf16_launches', 0)      # reduced modes only
    flop_per_step = (prof['gemm_flop'] + split_flop + bf_flop) / sampled
    step_s = elapsed / args.steps
    step_tf = flop_per_step / step_s / 1e12      # per GPU: every rank runs its own shard
    # time the two matrix pipes would need at their peaks for one step's launches: fp32 launches at the fp32 MFMA peak, the
    # split-bf16 launches (six bf16 products per fp32-equivalent product) at the dense bf16 peak
    t_min = ((prof['gemm_flop'] / sampled) / (PEAK_FP32_MFMA_TFLOPS * 1e12) + 6.0 * (split_flop / sampled) / (PEAK_BF16_MFMA_TFLOPS * 1e12)
             + (bf_flop / sampled) / (PEAK_BF16_MFMA_TFLOPS * 1e12))
    measured = ('HIP events around every GEMM launch of %d sampled steps of a single-stream pass (%d steps) after the timed region; '
                'rocprofv3 --kernel-trace --stats agrees with it on the one-context one-stream command (`bench.py --contexts 1 --streams 1`, '
                'profiles/r04_bench_streams1_kernel_stats.csv); with two contexts in flight the kernels of two steps overlap and a launch\'s '
                'duration as rocprofv3 sees it is longer, which is why the kernel-level figure comes from this pass' % (sampled, args.profile_steps))
    fp32 = {'kernel': 'mpe::k_linear_dma / k_linear_skinny* (fp32 MFMA 16x16x4; K stages by LDS-DMA from loader waves, fused bias + LeakyReLU): '
                      + ('fc1 of GAT layer 0 (head rows only, grouped by camera: K = 180 blocks)' if split_n else 'every mpe_linear launch of a step'),
            'achieved': achieved, 'peak': PEAK_FP32_MFMA_TFLOPS, 'unit': 'TFLOP/s', 'frac': achieved / PEAK_FP32_MFMA_TFLOPS,
            'launches': prof['gemm_launches'], 'avg_launch_ms': prof['gemm_ms'] / max(1, prof['gemm_launches']),
            'flop_per_step': prof['gemm_flop'] / sampled}
    if split_n:
        eq = split_flop / (split_ms * 1e-3) / 1e12
        main = {'kernel': 'mpe::k_linear_sb* (csrc/gemm_sb16.hip: nn.Linear with fp32 operands taken as three bf16 planes each, the six '
                          'significant partial products on v_mfma_f32_16x16x32_bf16, fp32 accumulators (+ f64 running sums every second K '
                          'stage in the MLP), activation tile and weight planes staged by LDS-DMA from loader waves (one persistent twelve-wave '
                          'workgroup per CU, 256-row tiles, ring of three K stages), fused bias + LeakyReLU '
                          '+ attention coefficients): the GAT launches of layers 1-4 and all MLP launches = %.0f %% of the GEMM time of a step'
                          % (100.0 * split_ms / max(1e-9, split_ms + prof['gemm_ms'])),
                'bound': 'mfma',
                'achieved': 6.0 * eq, 'peak': PEAK_BF16_MFMA_TFLOPS, 'unit': 'TFLOP/s', 'frac': 6.0 * eq / PEAK_BF16_MFMA_TFLOPS,
                'achieved_definition': 'EXECUTED bf16 matrix FLOP/s = 6 x the algorithmic 2*M*N*K of the launches / their time, against the dense '
                                       'bf16 MFMA peak (the pipe the kernel runs on)',
                'achieved_fp32_equivalent': eq, 'fp32_equivalent_vs_fp32_mfma_peak': eq / PEAK_FP32_MFMA_TFLOPS,
                'fp32_equivalent_note': 'algorithmic 2*M*N*K per second; the fp32 MFMA these launches ran on until round 3 peaks at %.1f '
                                        'TFLOP/s (they reached 105-116 there)' % PEAK_FP32_MFMA_TFLOPS,
                'launches': split_n, 'avg_launch_ms': split_ms / split_n, 'flop_per_step_fp32_equivalent': split_flop / sampled,
                'fp32_mfma_launches': fp32}
    else:
        main = dict(fp32, bound='mfma')
    bf16 = None
    if bf_n:
        bf_tf = bf_flop / (bf_ms * 1e-3) / 1e12
        bf16 = {'kernel': 'mpe::k_linear_bf16 (reduced precision, configs[4]: weights and staged activations in bf16, one bf16 product per product)',
                'bound': 'mfma', 'achieved': bf_tf, 'peak': PEAK_BF16_MFMA_TFLOPS, 'unit': 'TFLOP/s', 'frac': bf_tf / PEAK_BF16_MFMA_TFLOPS,
                'launches': bf_n, 'avg_launch_ms': bf_ms / bf_n, 'flop_per_step': bf_flop / sampled}
        if bf_ms > split_ms and bf_ms > prof['gemm_ms']:        # the bf16 launches carry the step: they are the dominant kernel of this run
            bf16['fp32_mfma_launches'] = fp32
            if split_n:
                bf16['split_bf16_launches'] = {k: main[k] for k in ('achieved', 'peak', 'frac', 'launches', 'avg_launch_ms') if k in main}
            main = bf16
        else:
            main['bf16_launches'] = bf16
    main.update({
        'traffic': traffic, 'traffic_source': src, 'measured': measured,
        'sampled_steps': sampled, 'flop_per_step': flop_per_step,
        'gemm_share_of_single_stream_step': ((gemm_s + split_ms * 1e-3 + bf_ms * 1e-3) / sampled) / (prof['single_stream_ms_per_step'] * 1e-3),
        'single_stream_ms_per_step': prof['single_stream_ms_per_step'],
        'step': {'achieved': step_tf, 'frac': t_min / step_s, 'unit': 'TFLOP/s',
                 'frac_against_fp32_peak': step_tf / PEAK_FP32_MFMA_TFLOPS,
                 'definition': 'achieved: algorithmic GEMM FLOPs (2*M*N*K, fp32-equivalent) of one step / wall time of one step of the '
                               'timed region (every kernel of the step, engine mode as in config.engine_mode).  frac: the time the matrix '
                               'pipes would need at their peaks for the step\'s launches (fp32 launches at %.1f TFLOP/s, split-bf16 '
                               'launches as six bf16 products and plain bf16 launches as one at %.0f TFLOP/s) / that wall time; frac_against_fp32_peak: achieved / the '
                               'fp32 MFMA peak, the figure of rounds 1-3 (equal to frac when no launch runs on the bf16 pipe)'
                               % (PEAK_FP32_MFMA_TFLOPS, PEAK_BF16_MFMA_TFLOPS)},
        'flop_definition': 'algorithmic 2*M*N*K of the launches (layer-0 edge-node rows de-duplicated); every launch is priced against the '
                           'peak of the pipe it runs on',
        'what_bounds_it': 'POWER: the in-kernel clock of the split-bf16 launches on real operands is 2.0 GHz (2.4 GHz with zero weights at the '
                          'same cycle count, profiles/r05_sb_clock.txt); the peak above is the 2.4 GHz figure',
        'roofline_note': 'frac = the dominant kernel\'s achieved / peak; frac_against_fp32_peak (in `step`) is a ratio of FLOP definitions, not a roofline fraction',

    })
    main['hbm'] = {'achieved': hbm_tbs, 'peak': PEAK_HBM_TBS, 'unit': 'TB/s', 'frac': hbm_tbs / PEAK_HBM_TBS,
                   'bytes_per_frame': bytes_per_frame,
                   'definition': 'compulsory bytes of the whole path per frame (packed input + poses + weights once per '
                                 'batch) x frames/s per GPU; tiny by construction: the path is MFMA-bound'}
    return main


def json_inclusive(args, torch, eng, wire, B, uniq, contexts=1):
    """SURVEY.md §8 f1 as a timed region: the reference's wire format -- one JSON document, a list of frames, per
    camera [json string of the skeleton list, timestamp, 'no_image', bodies_3D]
    (panoptic_conversor/get_joints_from_panoptic_model_multi.py:231-236,287) -- as BYTES in host memory ->
    Engine.stream_json: the host walks the first level only (frame extents by a parallel scan, camera keys, the extent of
    every skeleton string) and copies the strings into a page-locked buffer; one H2D copy per batch; the second level is
    parsed ON THE DEVICE (csrc/jsonparse.hip) on a side stream while the previous batch computes; match + 3D stage; D2H of
    the poses into pinned memory."""
    n_steps = args.json_steps
    one = [wire[i % uniq] for i in range(B)]
    body = json.dumps(one)[1:-1]
    text = ('[' + ','.join([body] * n_steps) + ']').encode()
    warm = ('[' + ','.join([body] * 2) + ']').encode()
    mode = args.mode
    assert sum(len(n) for _, _, n in eng.stream_json(warm, chunk_frames=B, mode=mode, contexts=contexts)) == 2 * B
    # one untimed pass over the document itself (the warm-up steps of this region): the first pass over freshly built bytes
    # measures the host's page and cache state as much as the pipeline (167-171 k against 180 k for every later pass)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    assert sum(len(n) for _, _, n in eng.stream_json(text, chunk_frames=B, mode=mode, contexts=contexts)) == n_steps * B
    torch.cuda.synchronize()
    cold = n_steps * B / (time.perf_counter() - t0)       # the FIRST pass over these bytes: what a stream that is read once sees
    for rep in range(int(os.environ.get('MPE_BENCH_JSON_REPEAT', '1'))):        # > 1: diagnostics (each repeat on stderr), the last one counts
        t0 = time.perf_counter()
        got = sum(len(n) for _, _, n in eng.stream_json(text, chunk_frames=B, mode=mode, contexts=contexts))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert got == n_steps * B
        if os.environ.get('MPE_BENCH_JSON_REPEAT'):
            print('json_inclusive repeat %d: %.1f frames/s' % (rep, got / dt), file=sys.stderr)
    threads = usable_cpus()
    return {'value': cold, 'value_warm': got / dt, 'unit': 'frames/s', 'ms_per_step': 1e3 * n_steps * B / cold / n_steps, 'steps': n_steps,
            'json_bytes_per_step': len(text) // n_steps, 'json_gb_per_s': len(text) * (cold / (n_steps * B)) / 1e9, 'host_threads_available': threads,
            'parser': 'device (csrc/jsonparse.hip); host: frame extents + string extents only',
            'warmup': 'value: the FIRST pass over the freshly built bytes, what a stream that is read once sees (two 2-batch calls before it '
                      'make the streams and buffers); value_warm: the second pass over the same document (page and cache state warm)',
            'what': 'wire-format frame JSON bytes in host memory -> first level on the host (parallel frame scan, skeleton strings '
                    'copied to a page-locked buffer) -> H2D -> second level parsed on the device -> match + 3D stage -> D2H of '
                    'poses into pinned host memory; batch i+1 is parsed while batch i computes'
                    + ('; batches take turns on %d contexts' % contexts if contexts > 1 else '')}


def usable_cpus():
    """CPUs this process may really use: the affinity mask cut by the cgroup CPU quota (a GPU box shows 256 CPUs and
    grants 16; an MKL pool sized to the 256 is throttled by the kernel for most of every 100 ms period)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        with open('/sys/fs/cgroup/cpu.max') as fh:
            q, per = fh.read().split()[:2]
        if q != 'max' and int(per) > 0:
            n = max(1, min(n, int(q) // int(per)))
    except (OSError, ValueError):
        pass
    return n


def pmc_traffic():
    """Fabric bytes per GEMM launch from the committed rocprofv3 PMC passes of this same command
    (separate FETCH_SIZE / WRITE_SIZE passes, gfx950 2x FETCH correction).  PMC cannot be sampled
    from inside the process: this is an OFFLINE measurement and says which file it came from."""
    for name in traffic_files():
        try:
            with open(os.path.join(ROOT, 'profiles', name)) as fh:
                d = json.load(fh)
                # the dominant kernel's launches: k_linear_sb (round 4 on), else all k_linear* launches
                return d.get('k_linear_sb_bytes_per_launch', d['k_linear_bytes_per_launch']), 'offline: profiles/' + name
        except (OSError, KeyError, ValueError):
            continue
    return None, None


def cpu_baseline_and_parity(args, np, torch, calib, params, lo, device):
    """CPU port (the oracle) timed on a bounded sample, rank 0 only; its results double as the parity sample.

    The sample is in the CAPTURE-VOLUME regime (SURVEY.md §8(d) parity fields; the 1e-3 mm item of the north star is
    about poses of a few metres): same frame shape as the timed workload (views x persons), detections carrying an
    identity cue (synthetic.FrameSpec(identity_prob=True)), the hand-built matcher network and the decoder MLP with
    dense hash noise on every weight -- correct clusters, poses inside the room, an MPJPE that means something.  The
    timed workload keeps its dense random weights: MFMA time does not depend on the values, board power does."""
    if args.cpu_sample <= 0:
        return None, None
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    onp = importlib.import_module('oracle_np')
    syn = importlib.import_module(PKG + '.synthetic')
    pipeline = importlib.import_module(PKG + '.pipeline')
    V, J = len(params.used_cameras_skeleton_matching), len(params.joint_list)
    nf = 2 + V * J * 10
    n = args.cpu_sample
    gat_sd = syn.matcher_gat_state_dict(nf, V, J, noise_seed=5, noise_bound=1e-4)
    prm = syn.gat_params(nf)
    mlp_sd = syn.decoder_mlp_state_dict(len(params.used_cameras), J, params.numbers_per_joint, noise_seed=3, noise_bound=0.01)
    spec = syn.FrameSpec(persons=min(args.persons, 8), identity_prob=True)       # the identity cue has eight levels
    frames, gts = [], []
    for i in range(n):
        f, gt = syn.make_frame(calib, lo + 100000 + i, spec)
        frames.append(onp.processed_input(f))
        gts.append(gt['persons'])
    eng = pipeline.Engine(params, calib, max_frames=n, max_persons_per_camera=args.persons, device=str(device))
    try:
        eng.load_gat(gat_sd, prm)
        eng.load_mlp(mlp_sd)
        had = torch.get_num_threads()
        cores = min(had, usable_cpus())
        torch.set_num_threads(cores)
        try:
            onp.run_frame(frames[0], calib, gat_sd, prm, mlp_sd, mode=args.mode)       # warm up
            res = []
            t0 = time.perf_counter()
            for i in range(n):
                res.append(onp.run_frame(frames[i], calib, gat_sd, prm, mlp_sd, mode=args.mode))
            dt = time.perf_counter() - t0
        finally:
            torch.set_num_threads(had)
        base = {'value': n / dt, 'unit': 'frames/s', 'cores': cores, 'kind': 'port',
                'sample': '%d frames of the workload\'s shape (%d views x %d persons), per-frame loop as in the reference '
                          '(torch-CPU GEMMs)' % (n, V, spec.persons)}
        db = eng.to_device(eng.pack(frames))
        scores, persons, n_persons = eng.match(db)
        if args.mode == 'mlp':
            poses = eng.mlp3d(db, persons, n_persons)[0]
        else:
            poses = eng.triangulate(db, persons, n_persons)[0]
        eng.sync_status()
        poses_ma = poses_fx = None
        if args.mode == 'mlp' and not (args.reduced or args.cfg4 or args.bf16_mlp):
            eng.set_precision(False, True, mlp_max_accuracy=True)              # the MLP's maximum-accuracy mode on the same persons
            poses_ma = eng.mlp3d(db, persons, n_persons)[0].cpu().numpy()
            eng.set_precision(False, True, mlp_f64=True)                       # ... and its reference-exact mode
            poses_fx = eng.mlp3d(db, persons, n_persons)[0].cpu().numpy()
            eng.set_precision(False, True)
        persons, n_persons, poses = persons.cpu().numpy(), n_persons.cpu().numpy(), poses.cpu().numpy()
        scores = scores.cpu().numpy()
        used = list(calib.params.used_joints)
        exact, max_abs, max_ulp, dscore, largest = 0, 0.0, 0.0, 0.0, 0.0
        e_gpu, e_cpu, gx, rx, gx_ma, d_ma, gx_fx, d_fx = [], [], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0

        def mpjpe(pred, gt_people):
            return min(float(np.mean([np.linalg.norm(pred[j] - g[j]) for j in used])) for g in gt_people)
        for f in range(n):
            r = res[f]
            if r is None:
                exact += int(n_persons[f] == 0)
                continue
            h0, H, e0, M = db.host.frame_counts(f)
            dscore = max(dscore, float(np.abs(scores[e0:e0 + M] - r['scores']).max()))
            want = np.array(r['persons'], np.int32).reshape(-1, V)
            if n_persons[f] != len(want) or not np.array_equal(persons[f, :len(want)], want):
                continue
            exact += 1
            if not len(want):
                continue
            if args.mode == 'mlp':
                ref = r['poses']
                # each side's distance from the network evaluated in f64 (fp32 between layers) on the oracle's rows
                ex = onp.mlp_exact(mlp_sd, r['mlp_in']).numpy().reshape(len(want), -1, 3) * 10.0
                gx = max(gx, float(np.abs(poses[f, :len(want)] - ex).max()))
                rx = max(rx, float(np.abs(ref - ex).max()))
                if poses_ma is not None:
                    gx_ma = max(gx_ma, float(np.abs(poses_ma[f, :len(want)] - ex).max()))
                    d_ma = max(d_ma, float(np.abs(poses_ma[f, :len(want)] - ref).max()))
                    gx_fx = max(gx_fx, float(np.abs(poses_fx[f, :len(want)] - ex).max()))
                    d_fx = max(d_fx, float(np.abs(poses_fx[f, :len(want)] - ref).max()))
            else:
                ref = np.stack([np.stack([t.get(j, np.zeros(3)) for j in range(eng.J)]) for t in r['tri']])
            d = np.abs(poses[f, :len(want)] - ref)
            max_abs = max(max_abs, float(d.max()))
            largest = max(largest, float(np.abs(ref).max()))
            row_ulp = np.spacing(np.abs(ref).reshape(len(want), -1).max(axis=1).astype(np.float32)).astype(np.float64)
            max_ulp = max(max_ulp, float((d.reshape(len(want), -1) / row_ulp[:, None]).max()))
            for k in range(len(want)):
                e_gpu.append(mpjpe(poses[f, k], gts[f]))
                e_cpu.append(mpjpe(ref[k], gts[f]))
    finally:
        eng.close()
    met = max_abs * 1e3 <= 1e-3
    parity = {'sample_frames': n, 'regime': 'capture volume: matcher GAT + decoder MLP with dense noise; largest |pose| %.2f m' % largest,
              'clusters_exact_frac': exact / n, 'max_abs_mm': max_abs * 1e3,
              'max_abs_ulp': max_ulp if args.mode == 'mlp' else None,
              'ref_vs_exact_mm': rx * 1e3 if args.mode == 'mlp' else None,
              'gpu_vs_exact_mm': gx * 1e3 if args.mode == 'mlp' else None,
              'mlp_max_accuracy': ({'gpu_vs_exact_mm': gx_ma * 1e3, 'max_abs_mm': d_ma * 1e3, 'within_1e-3_mm_of_exact': gx_ma * 1e3 <= 1e-3,
                                    'mode': 'mpe_set_precision MLP 4: the split-bf16 form with an f64 flush after every K stage; asserted on every '
                                            'capture-volume golden row of the four rigs by tests/test_gpu_stages.py::test_mlp_within_1e_3_mm_of_the_exact_network'}
                                   if poses_ma is not None else None),
              'mlp_f64_exact': ({'gpu_vs_exact_mm': gx_fx * 1e3, 'max_abs_mm': d_fx * 1e3, 'within_1e-3_mm_of_exact': gx_fx * 1e3 <= 1e-3,
                                 'mode': 'mpe_set_precision MLP 5: exact fp32 x fp32 products accumulated in f64 on the f64 matrix pipe (csrc/gemm_f64.hip) -- '
                                         'the network evaluated in f64 with fp32 rounding between layers; max_abs_mm is then the reference\'s own distance from it'}
                                if poses_ma is not None else None),
              'mpjpe_mm': float(np.mean(e_gpu)) * 1e3 if e_gpu else None,
              'delta_mpjpe_mm': (abs(float(np.mean(e_gpu)) - float(np.mean(e_cpu))) * 1e3) if e_gpu else None,
              'max_abs_score_diff': dscore,
              'north_star': {'clusters_exact': exact == n, 'delta_mpjpe_within_0.01_mm': bool(e_gpu) and abs(float(np.mean(e_gpu)) - float(np.mean(e_cpu))) * 1e3 <= 0.01,
                             '3d_within_1e-3_mm': ('met' if met else 'UNMET: the reference\'s own fp32 MLP (torch-CPU) is %.1e mm from the '
                                                   'exactly evaluated network on these rows, the HIP path %.1e mm' % (rx * 1e3, gx * 1e3))
                             if args.mode == 'mlp' else ('met' if met else 'UNMET')},
              'against': 'CPU oracle (oracle/oracle_np.py) on the same frames; ulp = fp32 ulp of the largest output of the pose; '
                         'exact = the MLP evaluated in f64 with fp32 rounding between layers (tests/test_gpu_stages.py::'
                         'test_mlp_capture_volume_regime_every_golden_row asserts the same quantities on the reference\'s own outputs)'}
    return base, parity


def dry_run(args, dist, dmod, world, rank, B, cap, total, strong):
    """Launch / rendezvous / sharding / all-gather without a GPU: stand-in results that encode
    the global frame index, checked after the gather on every rank."""
    import torch
    lo = rank * cap if strong else rank * B
    ok = True
    for _ in range(max(1, args.steps)):
        poses = torch.arange(lo, lo + B, dtype=torch.float32).view(-1, 1, 1, 1).expand(-1, 2, 18, 3).contiguous()
        n_p = (torch.arange(lo, lo + B, dtype=torch.int32) % 3)
        if world > 1:
            gp, gn = dmod.all_gather_results(dmod.pad_to(poses, cap), dmod.pad_to(n_p, cap), cap * world)
            for r in range(world):
                r_lo, r_hi, _ = dmod.shard_range(total, r, world) if strong else (r * B, (r + 1) * B, B)
                seg = gp[r * cap: r * cap + (r_hi - r_lo), 0, 0, 0]
                ok = ok and bool(torch.equal(seg, torch.arange(r_lo, r_hi, dtype=torch.float32)))
    if world > 1:
        flag = torch.tensor([1 if ok else 0])
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        ok = bool(flag.item())
    if rank == 0:
        print(json.dumps({'dry_run': True, 'value': None, 'n_gpus': world, 'world_size_seen': dist.get_world_size() if world > 1 else 1,
                          'scaling': 'strong' if strong else 'weak', 'frames_per_step_total': total,
                          'frames_this_rank': B, 'gather_ok': ok,
                          'launcher': 'bench.py spawn' if os.environ.get('MPE_BENCH_SPAWNED') else 'external'}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0 if ok else 1


def main():
    args = parse_args()
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        return launch_ranks(args)
    return run_rank(args)


if __name__ == '__main__':
    sys.exit(main())
