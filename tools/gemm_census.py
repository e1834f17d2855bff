"""Which GEMM launches does every precision mode make?  For each configuration one `match` + `mlp3d` under Engine.profile(True),
then profile_read()'s nine numbers: launches / FLOP / ms of the fp32 MFMA, the split-bf16 and the plain bf16 forms.  The launch counts
and the FLOP figures depend on the host-side dispatch alone (csrc/gemm_form.h, csrc/api.hip: gemm()), not on the machine: the output of
this tool is committed as tests/golden/harness/gemm_census.json and tests/test_gpu_stages.py holds every later dispatch to it.

    python tools/gemm_census.py [--out FILE]        (needs a GPU; no other MPE_* switch set)
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = '3d_multi_pose_estimator_amd'

# Engine.set_precision keywords.  The GAT settings run with the default MLP and the other way round.
GAT_SETTINGS = [
    ('default', {}),
    ('gat_acc64', {'gat_acc64': True}),
    ('attn_fp16', {'attn_fp16': True}),
    ('gat_split=False', {'gat_split': False}),
    ('gat_acc64+gat_split=False', {'gat_acc64': True, 'gat_split': False}),
    ('attn_fp16+gat_split=False', {'attn_fp16': True, 'gat_split': False}),
    ('gat_reduced', {'gat_reduced': True}),
]
MLP_SETTINGS = [
    ('default', {}),
    ('mlp_max_accuracy', {'mlp_max_accuracy': True}),
    ('mlp_f64', {'mlp_f64': True}),
    ('mlp_split=False', {'mlp_split': False}),
    ('(False, False)', {'mlp_acc64': False, 'mlp_split': False}),
    ('mlp_bf16', {'mlp_bf16': True}),
]
# the two switches that change the route of a launch, read per call by the library (None = unset)
ENVIRONMENTS = [{'MPE_LATENCY_PATH': lat, 'MPE_NO_COEF_EPILOGUE': epi} for lat in (None, '0') for epi in (None, '1')]
# 1 frame: the latency launches; 17: the first size past them; 40 reaches the tile kernels
BATCH_SIZES = (1, 17, 40)
COMPARED = ('gemm_launches', 'split_launches', 'bf16_launches', 'gemm_flop', 'split_flop', 'bf16_flop')


def frames(calib, n, persons=(4, 2, 5, 1, 3, 4, 6, 4), start=100):
    """The synthetic frames of tests/test_gpu_latency.py (same recipe), as the callers hand them over: cameras that saw nobody
    are dropped (metrics_from_model.py:182-191)."""
    syn = importlib.import_module(PKG + '.synthetic')
    out = []
    for i in range(n):
        spec = syn.FrameSpec(persons=persons[i % len(persons)], empty_cameras=('trackerc',) if i % 5 == 3 else (),
                             joint_drop=0.15 if i % 2 else 0.0)
        frame = syn.make_frame(calib, start + i, spec)[0]
        out.append({cam: [json.dumps(json.loads(v[0])), v[1]] for cam, v in frame.items() if json.loads(v[0])})
    return out


def label(kind, name, environment, n_frames):
    env = ','.join('%s=%s' % (k, v) for k, v in sorted(environment.items()) if v is not None) or '-'
    return '%s %s | %s | %d frames' % (kind, name, env, n_frames)


def census(eng, calib):
    """{label: profile_read()} over every configuration.  Leaves the engine's precision and the environment as it found them."""
    batches = {n: eng.to_device(eng.pack(frames(calib, n))) for n in BATCH_SIZES}
    saved = {k: os.environ.get(k) for k in ENVIRONMENTS[0]}
    out = {}
    try:
        for kind, settings in (('gat', GAT_SETTINGS), ('mlp', MLP_SETTINGS)):
            for name, kw in settings:
                eng.set_precision(**kw)
                for environment in ENVIRONMENTS:
                    for k, v in environment.items():
                        if v is None:
                            os.environ.pop(k, None)
                        else:
                            os.environ[k] = v
                    for n, db in batches.items():
                        eng.profile(True)
                        _, persons, n_persons = eng.match(db)
                        eng.mlp3d(db, persons, n_persons)
                        eng.profile(False)
                        out[label(kind, name, environment, n)] = eng.profile_read()
        eng.sync_status()
    finally:
        eng.set_precision()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None, help='write the JSON here instead of standard output')
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    syn = importlib.import_module(PKG + '.synthetic')
    params = importlib.import_module(PKG + '.parameters').parameters
    calib = importlib.import_module(PKG + '.calibration').Calibration(params)
    with open(os.path.join(ROOT, 'tests', 'golden', 'meta.json')) as fh:
        m = json.load(fh)                      # the deterministic weights of the test-suite's fixtures
    eng = importlib.import_module(PKG + '.pipeline').Engine(params, calib, max_frames=64, max_persons_per_camera=10)
    eng.load_gat(syn.gat_state_dict(m['gat_seed'], m['num_feats'], logit_gain=m['logit_gain'], logit_shift=m['logit_shift']),
                 syn.gat_params(m['num_feats']))
    eng.load_mlp(syn.mlp_state_dict(m['mlp_seed'], m['mlp_in']))
    text = json.dumps(census(eng, calib), indent=1)
    eng.close()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    else:
        print(text)


if __name__ == '__main__':
    main()
