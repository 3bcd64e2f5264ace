"""AdaGrad without a GPU: the fp64 restatement (tests/adagrad_ref.py) against torch.optim.Adagrad driven by torch-CPU
autograd of the fp64 hinge, the checkpoint round trip with the accumulator, and the driver's argument-time refusals."""
import numpy as np
import pytest
import torch

from tests import adagrad_ref as AR


def torch_hinge_sum(table, pos, neg, margin, max_norm):
    """SUM_i max(E(pos_i) - E(neg_i) + margin, 0) of holE.py:231 for the ComplEx score, clip_by_norm included."""
    k = table.shape[1] // 2

    def emb(ids):
        x = table[ids]
        inv = torch.rsqrt((x * x).sum(-1, keepdim=True))
        y = x * (torch.minimum(inv, torch.full_like(inv, 1.0 / max_norm)) * max_norm)
        return torch.complex(y[:, :k], y[:, k:])

    def ev(tr):
        h, t, r = emb(tr[:, 0]), emb(tr[:, 1]), emb(tr[:, 2])
        return torch.sigmoid((h * (r * torch.conj(t))).real.sum(1))
    return torch.clamp(ev(pos) - ev(neg) + margin, min=0.0).sum()


def test_restatement_equals_torch_adagrad_over_two_dependent_steps():
    rng = np.random.default_rng(5)
    N, d, B, lr, a0, margin = 12, 8, 9, 0.1, 0.1, 0.2
    table = rng.standard_normal((N, d)) * 0.25
    table[4] *= 6.0                                        # a row of norm > 1: the clip's Jacobian
    assert np.linalg.norm(table[4]) > 1 and np.linalg.norm(table[5]) < 1
    pos = np.stack([rng.integers(2, N, B), rng.integers(2, N, B), rng.integers(0, 2, B)], 1)
    pos[:3, 0] = 4                                         # duplicates: row 4 three times as head, two relation rows for 9 pairs
    neg = pos.copy()
    neg[:, 1] = rng.integers(2, N, B)
    neg[0] = pos[0]                                        # a pair whose negative is its positive
    accum = np.full((N, d), a0)
    param = torch.nn.Parameter(torch.tensor(table))
    opt = torch.optim.Adagrad([param], lr=lr, initial_accumulator_value=a0, eps=0)
    tp, tn = torch.as_tensor(pos), torch.as_tensor(neg)
    for _ in range(2):
        opt.zero_grad()
        torch_hinge_sum(param, tp, tn, margin, 1.0).backward()
        opt.step()
        loss, s, named = AR.step(table, accum, pos, neg, lr, margin)
        assert 0 < (loss > 0).sum() and np.abs(s[4]).max() > 0
        assert np.abs(param.detach().numpy() - table).max() < 1e-12
        assert np.abs(opt.state[param]["sum"].numpy() - accum).max() < 1e-12
    assert not np.array_equal(accum[4], np.full(d, a0))


def test_restatement_leaves_unnamed_rows_alone():
    table, accum = np.ones((5, 2)), np.full((5, 2), 0.1)
    s, named = AR.apply_rows(table, accum, [3, -1, 3, 7], np.array([[1., 2.], [9., 9.], [1., 0.], [5., 5.]]), 0.5)
    assert named.tolist() == [False, False, False, True, False]
    assert np.array_equal(accum[3], [0.1 + 4.0, 0.1 + 4.0]) and np.array_equal(table[[0, 1, 2, 4]], np.ones((4, 2)))
    assert np.allclose(table[3], 1.0 - 0.5 * 2.0 / np.sqrt(4.1))


def test_checkpoint_round_trip_with_the_accumulator(tmp_path):
    from graphembeddings_amd import train as T
    emb, acc = torch.arange(12, dtype=torch.float32).view(4, 3), torch.full((4, 3), 0.1) + torch.arange(3.0)
    T.save_checkpoint(str(tmp_path), emb, 17, acc)
    e, g, a = T.load_checkpoint(str(tmp_path), device="cpu", with_accumulator=True)
    assert g == 17 and torch.equal(e, emb) and torch.equal(a, acc)
    assert T.load_checkpoint(str(tmp_path), device="cpu")[1] == 17          # the old form still reads it
    # a checkpoint of the SGD loop holds none, and is the file it always was
    T.save_checkpoint(str(tmp_path), emb, 3)
    e, g, a = T.load_checkpoint(str(tmp_path), device="cpu", with_accumulator=True)
    assert g == 3 and a is None
    assert sorted(torch.load(T.checkpoint_path(str(tmp_path)), weights_only=True)) == ["embeddings", "global_step"]


def test_train_driver_refuses_adagrad_combinations_at_argument_time(monkeypatch):
    from graphembeddings_amd import train as T
    base = ["--data_dir", "d", "--output_dir", "o"]
    parse = lambda extra: T.build_parser().parse_args(base + extra)
    ok = parse(["--optimizer", "adagrad", "--adagrad_init", "0.5"])
    assert ok.optimizer == "adagrad" and ok.adagrad_init == 0.5 and parse([]).optimizer == "sgd" and parse([]).adagrad_init == 0.1
    T.check_optimizer_flags(ok)
    T.check_optimizer_flags(parse(["--log_loss", "--gpus", "2"]))           # SGD: nothing to refuse
    for extra, world in ((["--optimizer", "adagrad", "--log_loss"], 1), (["--optimizer", "adagrad", "--gpus", "2"], 1),
                         (["--optimizer", "adagrad"], 2), (["--optimizer", "adagrad", "--adagrad_init", "0"], 1)):
        with pytest.raises(SystemExit):
            T.check_optimizer_flags(parse(extra), world)
    with pytest.raises(SystemExit):
        parse(["--optimizer", "adam"])
    # main() refuses before it reads data, starts ranks or touches a GPU
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for extra in (["--optimizer", "adagrad", "--log_loss"], ["--optimizer", "adagrad", "--gpus", "2"]):
        with pytest.raises(SystemExit) as e:
            T.main(base + extra)
        assert "adagrad" in str(e.value)
