"""Writes tests/golden/pajigsaw_pairs.npz: the reference's ``Pajigsaw`` data set class (data/datasets/pajigsaw_dataset.py) run on a
small synthetic data set, its random draws fed from recorded uniforms.

    python tools/make_pajigsaw_golden.py --reference <checkout of glmanhtu/vit-ed>

The class is imported from the checkout, not copied.  ``cv2`` and ``torchvision.datasets.VisionDataset`` are not needed by anything
recorded here, so minimal stand-in modules are registered under those names before the import.  The data set is written to a
temporary directory: ``train.json`` with 3 images cut into grids of 2 x 3, 3 x 3 and 1 x 4 fragments (one fragment with
``white_percentage`` 0.9, one with a rotated duplicate of ``degree`` 90) and one tiny generated PNG per fragment.

``torch.rand`` and ``random.choice`` are replaced while ``__getitem__`` runs: ``torch.rand(1)`` returns the recorded u0, then u1;
``random.choice(seq)`` returns ``seq[min(int(u len), len - 1)]`` for u = u2 - except the draw from ``im_names``, which is handed the
image ``engine.pajigsaw_pair_plan`` names for u3: k = min(int(u3 (m - 1)), m - 2) among the m images, stepping over the sample's own
(the reference redraws until the image differs, which is the same distribution).

The file holds arrays only:
  json           uint8 [bytes]   the synthetic train.json (the tests' input; synthetic, no reference text)
  sample_path    str [n]         im_path of samples[i], in the reference's order
  im_names       str [m]
  pos_ptr / pos_path, neg_ptr / neg_path     the positive / negative lists of samples[i] as im_path strings, CSR over the samples
  ent_ptr / ent_path                         entries[im_names[k]] as im_path strings, CSR over im_names
  u              float64 [cases, 4]   the recorded uniforms
  case_sample    int64 [cases]        the sample number of each case
  second_path    str [cases]          the chosen second fragment
  labels         float32 [cases, 4]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'pajigsaw_pairs.npz')
GRIDS = {'img_b': (2, 3), 'img_a': (3, 3), 'img_c': (1, 4)}      # file order differs from the sorted order
WHITE = ('img_a', 1, 1)            # the centre of the 3 x 3 grid: skipped as a second fragment, still a sample
ROTATED = ('img_b', 0, 2)          # has a duplicate with degree 90 that is not a fragment


def synthetic_dataset():
    data = {}
    for name, (rows, cols) in GRIDS.items():
        frags = []
        for r in range(rows):
            for c in range(cols):
                frags.append({'im_path': f'{name}/r{r}c{c}.png', 'row': r, 'col': c, 'degree': 0,
                              'white_percentage': 0.9 if (name, r, c) == WHITE else round(0.05 * (r + c), 2)})
                if (name, r, c) == ROTATED:
                    frags.append({'im_path': f'{name}/r{r}c{c}_90.png', 'row': r, 'col': c, 'degree': 90, 'white_percentage': 0.1})
        data[name] = {'Fragment1v1Rotate90': frags}
    return data


def _install_standins():
    cv2 = types.ModuleType('cv2')
    cv2.COLOR_BGR2LAB, cv2.COLOR_LAB2BGR, cv2.BORDER_CONSTANT = 44, 56, 0
    cv2.cvtColor = lambda img, code: np.array(img, copy=True)
    cv2.imread = lambda path: np.zeros((8, 8, 3), np.uint8)
    sys.modules['cv2'] = cv2

    class VisionDataset:
        def __init__(self, root, transforms=None, transform=None, target_transform=None):
            self.root, self.transforms, self.transform, self.target_transform = root, transforms, transform, target_transform

    tv = types.ModuleType('torchvision')
    tvd = types.ModuleType('torchvision.datasets')
    tvd.VisionDataset = VisionDataset
    tv.datasets = tvd
    sys.modules['torchvision'], sys.modules['torchvision.datasets'] = tv, tvd


def uniforms(n_samples):
    """(sample, u) cases: a grid over all three branches for every sample, then the boundaries."""
    cases = []
    for s in range(n_samples):
        for u0 in (0.1, 0.9):
            for u1 in (0.2, 0.7):
                for u2 in (0.0, 0.35, 0.6, 0.9999999):
                    for u3 in (0.0, 0.49, 0.51, 0.9999999):
                        if u0 < 0.75 and (u1, u3) != (0.2, 0.0):
                            continue                      # a positive pair reads u0 and u2 only
                        cases.append((s, (u0, u1, u2, u3)))
    for s in (0, n_samples // 2, n_samples - 1):
        cases += [(s, (0.75, 0.1, 0.5, 0.5)), (s, (float(np.float32(0.7499999)), 0.1, 0.5, 0.5)), (s, (0.1, 0.1, 0.9999999, 0.5)),
                  (s, (0.8, 0.4999999, 0.9999999, 0.2)), (s, (0.8, 0.5, 0.3, 0.9999999))]
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    _install_standins()
    sys.path.insert(0, args.reference)
    import importlib.util
    spec = importlib.util.spec_from_file_location('pajigsaw_dataset', os.path.join(args.reference, 'data', 'datasets', 'pajigsaw_dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import torch
    from PIL import Image

    data = synthetic_dataset()
    text = json.dumps(data, indent=1)
    with tempfile.TemporaryDirectory() as root:
        with open(os.path.join(root, 'train.json'), 'w') as f:
            f.write(text)
        rng = np.random.default_rng(7)
        for name in data:
            os.makedirs(os.path.join(root, name))
            for frag in data[name]['Fragment1v1Rotate90']:
                Image.fromarray(rng.integers(0, 256, (6, 6, 3), dtype=np.uint8)).save(os.path.join(root, frag['im_path']))
        to_tensor = lambda img: torch.from_numpy(np.asarray(img).copy())
        ds = mod.Pajigsaw(root, mod._Split.TRAIN, transform=to_tensor)
        m = len(ds.im_names)

        def csr(lists):
            ptr = np.cumsum([0] + [len(v) for v in lists]).astype(np.int64)
            return ptr, np.array([e['im_path'] for v in lists for e in v], dtype=str)

        pos_ptr, pos_path = csr([s['positive'] for s in ds.samples])
        neg_ptr, neg_path = csr([s['negative'] for s in ds.samples])
        ent_ptr, ent_path = csr([ds.entries[name] for name in ds.im_names])
        cases = uniforms(len(ds))
        seconds, labels = [], []
        real_rand, real_choice, real_open = torch.rand, random.choice, Image.open
        opened = []

        class _Opened:
            def __init__(self, path):
                self.path = path

            def __enter__(self):
                opened.append(os.path.relpath(self.path, root))
                return real_open(self.path)

            def __exit__(self, *exc):
                return False

        try:
            mod.Image.open = _Opened
            for s, u in cases:
                draws = iter([u[0], u[1]])
                own = ds.im_names.index(ds.samples[s]['im_name'])
                k = min(int(u[3] * (m - 1)), m - 2)
                target = ds.im_names[k + (1 if k >= own else 0)]

                def fake_choice(seq, u=u, target=target):
                    if seq is ds.im_names:
                        return target
                    return seq[min(int(u[2] * len(seq)), len(seq) - 1)]

                torch.rand = lambda *a, draws=draws: torch.tensor([next(draws)], dtype=torch.float64)
                random.choice = fake_choice
                del opened[:]
                _, label = ds[s]
                assert opened[0] == ds.samples[s]['im_path']
                seconds.append(opened[1])
                labels.append(label.numpy())
        finally:
            torch.rand, random.choice, mod.Image.open = real_rand, real_choice, real_open
    labels = np.stack(labels).astype(np.float32)
    branches = {(tuple(l) != (0, 0, 0, 0)) for l in labels}
    assert branches == {True, False} and {int(l.argmax()) for l in labels if l.any()} == {0, 1, 2, 3}, 'not every label was reached'
    np.savez_compressed(GOLDEN, json=np.frombuffer(text.encode(), dtype=np.uint8), sample_path=np.array([s['im_path'] for s in ds.samples], dtype=str),
                        im_names=np.array(ds.im_names, dtype=str), pos_ptr=pos_ptr, pos_path=pos_path, neg_ptr=neg_ptr, neg_path=neg_path,
                        ent_ptr=ent_ptr, ent_path=ent_path, u=np.array([u for _, u in cases], dtype=np.float64),
                        case_sample=np.array([s for s, _ in cases], dtype=np.int64), second_path=np.array(seconds, dtype=str), labels=labels)
    print(f'wrote {GOLDEN}: {len(ds)} samples of {m} images, {len(cases)} cases, {os.path.getsize(GOLDEN)} bytes')


if __name__ == '__main__':
    main()
