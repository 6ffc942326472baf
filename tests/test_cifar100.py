"""CIFAR-100: the data set class (python and binary formats, download through data/download.py
from a file:// mirror), the trainer's data-set switch (class count, checkpoint names, top-5) and
the CLI switch.  CPU only; nothing here touches the network or the real archive's MD5s."""
import hashlib
import json
import os
import pickle
import sys
import tarfile

import numpy as np
import pytest

from faster_distributed_training_amd.data import cifar as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TRAIN, N_TEST = 24, 8
NAMES = [f"class_{i:02d}" for i in range(100)]


def _samples():
    rng = np.random.RandomState(11)
    n = N_TRAIN + N_TEST
    data = rng.randint(0, 256, (n, 3072)).astype(np.uint8)  # rows of 3 x 32 x 32, channel-major
    fine = rng.randint(0, 100, n)
    fine[:3] = (99, 0, 57)
    return data, fine, fine // 5


def _md5(path):
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def write_python_format(root):
    """cifar-100-python/{train,test,meta} under root; returns {file name: md5}."""
    data, fine, coarse = _samples()
    d = os.path.join(str(root), "cifar-100-python")
    os.makedirs(d)
    md5 = {}
    for name, sl in (("train", slice(0, N_TRAIN)), ("test", slice(N_TRAIN, None))):
        entry = {"data": data[sl], "fine_labels": [int(v) for v in fine[sl]], "coarse_labels": [int(v) for v in coarse[sl]],
                 "filenames": [f"img_{i}.png" for i in range(len(fine[sl]))], "batch_label": f"{name}ing batch 1 of 1"}
        with open(os.path.join(d, name), "wb") as f:
            pickle.dump(entry, f, protocol=2)
        md5[name] = _md5(os.path.join(d, name))
    with open(os.path.join(d, "meta"), "wb") as f:
        pickle.dump({"fine_label_names": NAMES, "coarse_label_names": [f"super_{i}" for i in range(20)]}, f, protocol=2)
    md5["meta"] = _md5(os.path.join(d, "meta"))
    return md5


def write_binary_format(root):
    data, fine, coarse = _samples()
    d = os.path.join(str(root), "cifar-100-binary")
    os.makedirs(d)
    rows = np.concatenate([coarse[:, None].astype(np.uint8), fine[:, None].astype(np.uint8), data], axis=1)
    assert rows.shape[1] == 3074
    rows[:N_TRAIN].tofile(os.path.join(d, "train.bin"))
    rows[N_TRAIN:].tofile(os.path.join(d, "test.bin"))


def _expect(train):
    data, fine, _ = _samples()
    sl = slice(0, N_TRAIN) if train else slice(N_TRAIN, None)
    return data[sl].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1), fine[sl]


def _check_loaded(root):
    for train in (True, False):
        ds = C.CIFAR100(str(root), train=train)
        img, lab = _expect(train)
        assert ds.data.dtype == np.uint8 and ds.data.shape == (len(lab), 32, 32, 3) and ds.data.flags.c_contiguous
        assert np.array_equal(ds.data, img) and np.array_equal(ds.targets, lab) and ds.targets.dtype == np.int64
        assert len(ds) == len(lab)
    x, t = C.CIFAR100(str(root), train=True, target_transform=lambda v: v + 1)[0]
    assert tuple(x.shape) == (3, 32, 32) and t == 100  # fine label 99, not coarse 19
    assert np.allclose(x.permute(1, 2, 0).numpy() * 255.0, _expect(True)[0][0])


def test_python_format(tmp_path):
    write_python_format(tmp_path)
    _check_loaded(tmp_path)
    assert C.get_classes("cifar100", str(tmp_path)) == tuple(NAMES)
    assert C.get_classes() == C.CLASSES and C.get_classes("cifar10") == C.CLASSES and len(C.CLASSES) == 10
    assert C.CIFAR100.num_classes == 100 and C.DATASETS == {"cifar10": C.CIFAR10, "cifar100": C.CIFAR100}
    with pytest.raises(ValueError):
        C.get_classes("imagenet")


def test_pickle_with_foreign_global_is_refused(tmp_path):
    write_python_format(tmp_path)
    with open(tmp_path / "cifar-100-python" / "train", "wb") as f:
        pickle.dump({"data": os.getcwd, "fine_labels": []}, f, protocol=2)  # a reference to posix.getcwd
    with pytest.raises(pickle.UnpicklingError, match="refusing to load"):
        C.CIFAR100(str(tmp_path), train=True)
    with open(tmp_path / "cifar-100-python" / "meta", "wb") as f:
        pickle.dump({"fine_label_names": os.getcwd}, f, protocol=2)
    with pytest.raises(pickle.UnpicklingError, match="refusing to load"):
        C.get_classes("cifar100", str(tmp_path))


def test_binary_format_loads_identically(tmp_path):
    write_binary_format(tmp_path)
    _check_loaded(tmp_path)
    (tmp_path / "cifar-100-binary" / "fine_label_names.txt").write_text("\n".join(NAMES) + "\n")
    assert C.get_classes("cifar100", str(tmp_path)) == tuple(NAMES)


@pytest.fixture
def mirror(tmp_path, monkeypatch):
    """A file:// mirror holding a tar.gz of the fixture, with the module's CIFAR-100 URL / MD5
    constants pointed at it; returns the (empty) data root."""
    src = tmp_path / "mirror"
    md5 = write_python_format(src)
    tgz = str(src / "cifar-100-python.tar.gz")
    with tarfile.open(tgz, "w:gz") as tf:
        tf.add(str(src / "cifar-100-python"), arcname="cifar-100-python")
    monkeypatch.setattr(C, "C100_URL", "file://" + tgz)
    monkeypatch.setattr(C, "C100_TGZ_MD5", _md5(tgz))
    monkeypatch.setattr(C, "C100_TRAIN_LIST", [("train", md5["train"])])
    monkeypatch.setattr(C, "C100_TEST_LIST", [("test", md5["test"])])
    monkeypatch.setattr(C, "C100_META", ("meta", md5["meta"]))
    return tmp_path / "data"


def test_download_verify_extract_load(mirror, monkeypatch):
    ds = C.CIFAR100(str(mirror), train=True, download=True)
    assert np.array_equal(ds.targets, _expect(True)[1]) and ds._check_integrity()
    assert os.path.isfile(mirror / "cifar-100-python.tar.gz") and os.path.isfile(mirror / "cifar-100-python" / "meta")
    _check_loaded(mirror)
    # present and intact: nothing is fetched again
    from faster_distributed_training_amd.data import download as D
    monkeypatch.setattr(D, "_urlretrieve", lambda *a, **k: (_ for _ in ()).throw(AssertionError("fetched again")))
    os.remove(mirror / "cifar-100-python.tar.gz")
    C.CIFAR100(str(mirror), train=False, download=True)


def test_download_md5_mismatch_is_an_error(mirror, monkeypatch):
    monkeypatch.setattr(C, "C100_TGZ_MD5", "0" * 32)
    with pytest.raises(RuntimeError, match="corrupted"):
        C.CIFAR100(str(mirror), train=True, download=True)
    assert not os.path.isdir(mirror / "cifar-100-python")


def test_missing_data_without_download_raises(tmp_path):
    with pytest.raises(RuntimeError, match="CIFAR-100 not found"):
        C.CIFAR100(str(tmp_path), train=True)
    with pytest.raises(RuntimeError, match="CIFAR-10 not found"):
        C.CIFAR10(str(tmp_path), train=True)


# ------------------------------------------------------------------ trainer
# the keys of the two JSONL records a CIFAR-10 epoch with evaluation writes, taken from a run of
# this configuration on the commit before the data-set switch
TRAIN_KEYS = ['epoch', 'epoch_time_s', 'img_per_s', 'lr', 'peak_mem_gb', 'skipped_steps', 'steps', 'time',
              'train_acc', 'train_loss']
TEST_KEYS = ['epoch', 'test_acc', 'time']


def _cfg(tmp_path, log, **kw):
    from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig
    base = dict(arch="resnet18", bs=8, epoch=1, synthetic=True, eval=True, plot=False, steps_per_epoch=2,
                checkpoint_dir=str(tmp_path), optimizer="madgrad", seed=7, log_path=str(tmp_path / log),
                save_last=True, extra={"subset_stride": 50})
    base.update(kw)
    return ResNetConfig(**base)


def _records(path):
    with open(path) as f:
        return [json.loads(line) for line in f]


def test_trainer_dataset_switch(tmp_path, capsys):
    from faster_distributed_training_amd.train.resnet_trainer import ResNetConfig, ResNetTrainer
    cfg = _cfg(tmp_path, "c100.jsonl", dataset="cifar100")
    assert cfg.num_classes == 100
    t = ResNetTrainer(cfg).fit()
    assert t.model.fc.out_features == 100 and int(t.train_loader.labels.max()) > 9
    assert os.path.basename(t.ckpt_path) == "resnet_cifar100_ckpt.pth" and os.path.isfile(t.ckpt_path)
    assert os.path.basename(t.last_path) == "resnet_cifar100_last.pth" and os.path.isfile(t.last_path)
    assert not os.path.exists(tmp_path / "resnet_ckpt.pth") and not os.path.exists(tmp_path / "resnet_last.pth")
    tr, te = _records(tmp_path / "c100.jsonl")
    assert sorted(tr) == TRAIN_KEYS and sorted(te) == sorted(TEST_KEYS + ["test_top5"])
    assert 0.0 < te["test_acc"] <= te["test_top5"] <= 100.0  # (test_acc > 0: the checkpoint above was written)
    assert "top-5" in capsys.readouterr().out
    stamp = os.path.getmtime(t.ckpt_path), os.path.getmtime(t.last_path)
    # a CIFAR-10 run in the same directory: its own files, today's records
    t10 = ResNetTrainer(_cfg(tmp_path, "c10.jsonl")).fit()
    assert t10.cfg.num_classes == 10 and t10.model.fc.out_features == 10
    assert os.path.basename(t10.ckpt_path) == "resnet_ckpt.pth" and os.path.isfile(t10.ckpt_path)
    assert os.path.isfile(tmp_path / "resnet_last.pth")
    assert stamp == (os.path.getmtime(t.ckpt_path), os.path.getmtime(t.last_path))
    tr, te = _records(tmp_path / "c10.jsonl")
    assert sorted(tr) == TRAIN_KEYS and sorted(te) == TEST_KEYS
    assert "top-5" not in capsys.readouterr().out
    # a 100-class run resumes from its own file only
    assert ResNetTrainer(_cfg(tmp_path, "r.jsonl", dataset="cifar100", resume=True, eval=False)).model.fc.out_features == 100
    with pytest.raises(ValueError, match="100 classes"):
        ResNetConfig(dataset="cifar100", num_classes=10)
    with pytest.raises(ValueError, match="dataset"):
        ResNetConfig(dataset="cifar1000")
    assert ResNetConfig(dataset="cifar100", num_classes=100).num_classes == 100
    assert ResNetConfig(num_classes=100, synthetic=True).num_classes == 100  # (still allowed on synthetic data)


def test_trainer_reads_cifar100_files(tmp_path):
    """Not synthetic: _build_data picks CIFAR100.  The files are in place and the module constants
    carry the fixture's MD5s, so rank 0's download=True finds them intact and fetches nothing."""
    from faster_distributed_training_amd.train.resnet_trainer import ResNetTrainer
    md5 = write_python_format(tmp_path / "data")
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(C, "C100_TRAIN_LIST", [("train", md5["train"])])
        mp.setattr(C, "C100_TEST_LIST", [("test", md5["test"])])
        mp.setattr(C, "C100_META", ("meta", md5["meta"]))
        mp.setattr(C, "C100_URL", "file:///nonexistent/cifar-100-python.tar.gz")
        t = ResNetTrainer(_cfg(tmp_path, "f.jsonl", dataset="cifar100", synthetic=False, extra={}, save_last=False,
                               data_root=str(tmp_path / "data")))
    finally:
        mp.undo()
    assert t.train_loader.n == N_TRAIN and t.test_loader.n == N_TEST
    assert np.array_equal(t.train_loader.labels.cpu().numpy(), _expect(True)[1])


# ------------------------------------------------------------------ CLI
def test_cli_dataset_switch(capsys):
    sys.path.insert(0, ROOT)
    try:
        import resnet50_test
        import resnet_infer
    finally:
        sys.path.remove(ROOT)
    a, base = resnet_infer.parse(["--dataset", "cifar100", "--synthetic"])
    cfg = resnet_infer.config_from_args(a, base)
    assert cfg.dataset == "cifar100" and cfg.num_classes == 100 and cfg.synthetic
    a, base = resnet_infer.parse(["--synthetic", "--bs", "64"])
    cfg = resnet_infer.config_from_args(a, base)
    assert cfg.dataset == "cifar10" and cfg.num_classes == 10 and cfg.bs == 64
    with pytest.raises(SystemExit):
        resnet_infer.parse(["--dataset", "cifar1000"])
    assert "invalid choice" in capsys.readouterr().err
    with pytest.raises(SystemExit):  # the reference-compatible CLI keeps the reference's flags
        resnet50_test.parse(["--dataset", "cifar100"])
    assert "unrecognized arguments" in capsys.readouterr().err
