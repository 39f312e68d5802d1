"""Write a database's `*_pseudotheta.pt` on MI355X (the reference's lib/data_utils/pseudo_theta.py:39-107).

    python tools/make_pseudotheta.py --db data/preprocessed_data/3dpw_test_db.pt --vibe-ckpt data/vibe_data/vibe_model_w_3dpw.pth.tar \
        --base-data data/base_data [--chunk 450] [--out data/preprocessed_data/3dpw_test_pseudotheta.pt]
    python tools/make_pseudotheta.py --check --db ... --vibe-ckpt ... --base-data ...
        # no GPU: which files are there, the db's columns and shapes, its videos, the chunks by length and the rows of every forward

The model is the one pseudo_theta.py:46-60 builds -- VIBE(seqlen=16, n_layers=2, hidden_size=1024, add_linear=True, use_residual=True), the
checkpoint's `gen_state_dict` loaded non-strictly, eval mode -- with the SMPL tables and mean parameters of `--base-data`; the chunks and their
order are `tepose_amd.prepare.pseudo_theta_schedule`, the forwards `tepose_amd.prepare.pseudo_theta`.  The output is the bare
[N,85] float32 array, joblib-dumped next to the database unless `--out` says otherwise.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tepose_amd import prepare  # noqa: E402

BASE_FILES = ('J_regressor_h36m.npy', 'J_regressor_extra.npy', 'smpl_mean_params.npz', 'SMPL_NEUTRAL.pkl')


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Pseudo-theta of a preprocessed database (joblib `*_db.pt`).  The h5 branch of the reference script '
                                             '(`insta_train_db.h5`) is out of scope: convert such a database to the joblib layout first.')
    ap.add_argument('--db', required=True, help='the `*_db.pt` to read: needs the columns vid_name and features [N,2048]')
    ap.add_argument('--vibe-ckpt', required=True, help='VIBE checkpoint with a gen_state_dict (the reference downloads vibe_model_w_3dpw.pth.tar)')
    ap.add_argument('--base-data', default='data/base_data', help='directory with %s' % ', '.join(BASE_FILES))
    ap.add_argument('--chunk', type=int, default=450, help='frames per VIBE forward (--vibe_batch_size of the reference script)')
    ap.add_argument('--max-rows', type=int, default=16384, help='chunks of equal length ride in one forward of at most this many rows')
    ap.add_argument('--out', help='default: the --db path with _db.pt replaced by _pseudotheta.pt')
    ap.add_argument('--check', action='store_true', help='report readiness and the schedule on the CPU, compute nothing')
    return ap.parse_args(argv)


def out_path(args):
    if args.out:
        return args.out
    if not args.db.endswith('_db.pt'):
        raise SystemExit('--db does not end in _db.pt: name the output with --out')
    return args.db[:-len('_db.pt')] + '_pseudotheta.pt'


def check_report(args):
    """Found / missing inputs, the db's columns, and the forwards a run would issue.  CPU only."""
    paths = [args.db, args.vibe_ckpt] + [os.path.join(args.base_data, f) for f in BASE_FILES]
    rep = {'found': [p for p in paths if os.path.isfile(p)], 'missing': [p for p in paths if not os.path.isfile(p)], 'chunk': args.chunk,
           'max_rows': args.max_rows, 'out': args.out or (out_path(args) if args.db.endswith('_db.pt') else None)}
    if os.path.isfile(args.db):
        import joblib
        db = joblib.load(args.db)
        rep['columns'] = {k: list(np.asarray(v).shape) for k, v in db.items()}
        try:
            sched = prepare.pseudo_theta_schedule(db['vid_name'], args.chunk)
            chunks = {(int(a), int(b)) for a, b, _ in sched}
            by_len = {}
            for _, length in chunks:
                by_len[length] = by_len.get(length, 0) + 1
            calls = prepare.forwards_of(db['vid_name'], args.chunk, args.max_rows)
            rep.update(frames=int(len(sched)), videos=int(len(np.unique(np.asarray(db['vid_name'])))), chunks=len(chunks),
                       chunks_by_length={str(k): by_len[k] for k in sorted(by_len, reverse=True)},
                       forwards=len(calls), rows_per_forward=[T * B for T, B in calls])
            f = np.asarray(db['features'])
            if f.shape != (len(sched), 2048):
                rep['error'] = 'features is %s, want [%d, 2048]' % (list(f.shape), len(sched))
        except (KeyError, ValueError) as e:
            rep['error'] = '%s: %s' % (type(e).__name__, e)
    if os.path.isfile(args.vibe_ckpt):
        from tepose_amd.data import load_checkpoint
        ck = load_checkpoint(args.vibe_ckpt)
        rep['checkpoint_tensors'] = len(ck['gen_state_dict'] if 'gen_state_dict' in ck else ck)
        if 'performance' in ck:
            rep['performance'] = float(ck['performance'])
    rep['ready'] = not rep['missing'] and 'error' not in rep
    return rep


def main(argv=None):
    args = parse_args(argv)
    if args.check:
        print(json.dumps(check_report(args)))
        raise SystemExit(0)
    import joblib
    import torch
    from tepose_amd.data import load_base_data, load_checkpoint, load_generator_state_dict
    from tepose_amd.smpl import SMPL
    from tepose_amd.vibe import VIBE
    out = out_path(args)
    base = load_base_data(args.base_data)
    ck = load_checkpoint(args.vibe_ckpt)
    if 'performance' in ck:
        print('Performance of pretrained model on 3DPW: %s' % (ck['performance'],))
    del ck
    model = VIBE(seqlen=16, n_layers=2, hidden_size=1024, add_linear=True, use_residual=True, pretrained='',
                 smpl=SMPL.from_tables(base['smpl_tables']), smpl_mean_params=base['mean_params'])
    model.load_state_dict(load_generator_state_dict(args.vibe_ckpt), strict=False)
    model = model.cuda().eval()
    db = joblib.load(args.db)
    calls = prepare.forwards_of(db['vid_name'], args.chunk, args.max_rows)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    thetas = prepare.pseudo_theta(model, db['features'], db['vid_name'], args.chunk, args.max_rows)
    dt = time.perf_counter() - t0
    joblib.dump(thetas, out)
    print(json.dumps({'out': out, 'frames': int(thetas.shape[0]), 'forwards': len(calls), 'rows_per_forward': [T * B for T, B in calls],
                      'seconds': round(dt, 3)}))


if __name__ == '__main__':
    main()
