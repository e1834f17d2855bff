"""TEST INFRASTRUCTURE (build container only): pin `--showgt` of the reprojection harness with what the REFERENCE'S OWN
SCRIPT prints.

The committed tests/golden/harness/syn_pinning_test.json makes test/reprojection_error.py skip every frame under
--showgt: its bodies carry '-1' in place of joint '2', so none is complete (:223-233).  This tool applies
harness/reprojection.py:add_joint2_from_minus1 in memory, writes the derived file to a temporary directory under the
same name (the name gives the calibration file tm_syn_pinning.pickle, :163-165), runs the reference script UNCHANGED
with --showgt on it (layout, stand-ins and weights of oracle/gen_harness_golden.py) and stores the parsed report in
tests/golden/harness/reprojection_showgt_expected.json.  The derived input is not committed: the tests apply the same
transform to the committed file.  (It lives beside the checkers, not under tools/: the diagnostics there stay clear of
the reference-running infrastructure, tests/test_host_logic.py::test_tools_do_not_use_the_oracle.)

    python tests/checkers/gen_reprojection_showgt_golden.py
"""
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gen_harness_golden as ghg  # noqa: E402

SCRIPT = 'reprojection_error.py'


def run_reference_showgt(data_file, tm_dir, models_dir):
    """ghg.run_reference's layout and environment, with --showgt on the command line."""
    layout = os.path.dirname(models_dir.rstrip('/'))
    os.makedirs(os.path.join(layout, 'test'), exist_ok=True)
    for name in ('tm_panoptic.pickle', 'human_pose.json'):
        link = os.path.join(layout, name)
        if not os.path.exists(link):
            os.symlink(os.path.join(ghg.REF, name), link)
    paths = [ghg.SHIMS, os.path.join(ghg.REF, 'skeleton_matching'), os.path.join(ghg.REF, 'utils'), ghg.REF]
    code = ('import sys, runpy; sys.dont_write_bytecode = True; sys.path[:0] = %r; '
            'sys.argv = [%r, "--testfiles", %r, "--showgt", "--tmdir", %r, "--modelsdir", %r, "--datastep", %r]; '
            'runpy.run_path(%r, run_name="__main__")'
            % (paths, SCRIPT, data_file, tm_dir, models_dir, str(ghg.DATASTEP), os.path.join(ghg.REF, 'test', SCRIPT)))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1', HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    res = subprocess.run([sys.executable, '-c', code], cwd=os.path.join(layout, 'test'), env=env, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError('%s failed:\n%s' % (SCRIPT, res.stderr[-3000:]))
    return res.stdout


def main():
    syn = importlib.import_module(ghg.PKG + '.synthetic')
    par = importlib.import_module(ghg.PKG + '.parameters')
    rp = importlib.import_module(ghg.PKG + '.harness.reprojection')
    params = par.parameters
    V, J = len(params.camera_names), len(params.joint_list)
    frames = json.load(open(os.path.join(ghg.OUT, ghg.TEST_NAME), 'rb'))
    changed = rp.add_joint2_from_minus1(frames)
    with tempfile.TemporaryDirectory() as layout:
        data_dir = os.path.join(layout, 'data')
        os.makedirs(data_dir)
        data_file = os.path.join(data_dir, ghg.TEST_NAME)
        with open(data_file, 'w') as fh:
            json.dump(frames, fh)
        shutil.copy(os.path.join(ghg.OUT, 'tm_syn_pinning.pickle'), data_dir)
        mdir = os.path.join(layout, 'models_panoptic')
        os.makedirs(mdir)
        ghg.save_models(mdir, syn, V, J)
        text = run_reference_showgt(data_file, data_dir, mdir)
    print(text)
    report = {'reprojection_error': ghg.parse_reprojection(text),
              'inputs': {'testfile': ghg.TEST_NAME, 'transform': rp.TRANSFORM_NAME, 'bodies_changed': changed,
                         'datastep': ghg.DATASTEP, 'showgt': True}}
    assert len(report['reprojection_error']) == V, text
    assert all(set(rows) == {'est', 'GT', 'triang'} for rows in report['reprojection_error'].values()), text
    with open(os.path.join(ghg.OUT, 'reprojection_showgt_expected.json'), 'w') as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == '__main__':
    main()
