"""Training / inference driver with the reference's CLI contract (holE.py:585-622).

  python -m graphembeddings_amd.train --data_dir D --output_dir O [--embedding_dim 200 ...]

Same flag names, defaults and meaning as holE.py:598-621.  What is reproduced is the BEHAVIOUR of
run_training (holE.py:249-370): batch_count = triple_count // batch_size; an "epoch" is
batch_count-1 steps (holE.py:340); lr = inverse_time_decay over learning_decay_steps epochs
(holE.py:292-294); 16 times per epoch the mean hinge of ONE random validation batch with fresh random
negatives is printed (holE.py:351-354) and the table is saved when it improves on the pocket loss,
which starts at 2.0 (holE.py:329, 357-360); the output directory must not exist unless
--resume_checkpoint (holE.py:254-255).  TF mechanics (queues, sessions, summaries, the V2
checkpoint bundle) are not: the table is saved as `model.ckpt.pt` (embeddings + global_step).
Between validation ticks the steps are enqueued natively by ge_train_steps (hinge) or
ge_train_steps_logloss (--log_loss) -- no Python per step.
Extras: --model hole (README.md:42 score), --seed, --max_steps, --checkpoint_seconds, --optimizer adagrad
(AdagradOptimizer in place of holE.py:296's GradientDescentOptimizer: ge_train_steps_adagrad; the checkpoint then also
holds `adagrad_accumulator`), --objective softmax (1-vs-all multiclass log-loss over all entities, both sides:
hole.SoftmaxTrainer on ge_softmax_grad; ComplEx with AdaGrad on one GPU, no validation ticks by default; --softmax_samples
K': sampled softmax, K' shared candidates a step on ge_softmax_sampled_grad; --softmax_candidate_sets types|observed: each
row's softmax over its relation's candidate set, ge_softmax_masked_grad; --softmax_labels all: one row per distinct query
with all its training answers as labels, ge_softmax_labels_grad; --softmax_validation_ticks T: T ticks per epoch on the
filtered MRR of --infer over the validation triples (of --infer --candidate_sets with --softmax_candidate_sets), each one
native call -- evaluate.RankPocket on ge_rank_validation_tick -- that keeps the best table and accumulator in a device
pocket, which model.ckpt.pt then follows (key `validation_mrr`); --softmax_validation_rows n ranks a seeded sample of
the validation triples; --softmax_patience P stops after P ticks in a row without an improvement).
"""
from __future__ import annotations

import argparse
import errno
import os
import sys
import time

import numpy as np
import torch

from . import data as D
from . import evaluate as E
from . import hole as H


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    p.add_argument('--learning_rate', type=float, default=0.1, help='Initial learning rate.')
    p.add_argument('--learning_decay_steps', type=float, default=32, help='Learning rate decay steps (in epochs).')
    p.add_argument('--learning_decay_rate', type=float, default=0.5, help='Learning decay rate.')
    p.add_argument('--batch_size', type=int, default=512, help='Batch size.')
    p.add_argument('--num_epochs', type=int, default=1000, help='Number of training epochs.')
    p.add_argument('--embedding_dim', type=int, default=128, help='Embedding dimension.')
    p.add_argument('--log_loss', action='store_true', help='Use logistic loss istead of pairwise ranking loss.')
    p.add_argument('--l2_regularization', type=float, default=0.1, help='L2 regularization weight (log loss only).')
    p.add_argument('--negative_ratio', type=int, default=1, help='Number of negative labels sampled in log_loss.')
    p.add_argument('--margin', type=float, default=0.2, help='Hinge loss margin.')
    p.add_argument('--padded_size', type=int, default=1024,
                   help='The maximum number of entities to use for each type while sampling corrupt triples.')
    p.add_argument('--output_dir', type=str, required=True, help='Output (checkpoint) directory.')
    p.add_argument('--data_dir', type=str, required=True, help='Input data directory.')
    p.add_argument('--reader_threads', type=int, default=4, help='Accepted for compatibility; ingest is one pass.')
    p.add_argument('--resume_checkpoint', action='store_true', help='Resume training on the checkpoint model.')
    p.add_argument('--save_embeddings', action='store_true', help='Output the embeddings to stdout.')
    p.add_argument('--infer', action='store_true', help='Link-prediction evaluation from the latest checkpoint.')
    p.add_argument('--infer_threshold', type=float, default=0.05, help='Max loss to save triples')
    p.add_argument('--predict_k', type=int, default=0,
                   help='With --infer: also write <output_dir>/inference_results.tsv, every pop up to the K-th filtered '
                        'prediction of each confident (head, relation) test query (0: no predictions).')
    p.add_argument('--candidate_sets', choices=['types', 'observed'], default=None,
                   help='With --infer: also rank every test triple against its relation\'s own candidate set (types: every '
                        'entity whose type was seen on that side of the relation in train + valid; observed: the entities seen '
                        'there) and print a "constrained:" line; --predict_k then predicts from the tail sets only.')
    p.add_argument('--relation_ranks', action='store_true',
                   help='With --infer: also rank every test triple\'s relation among all relation rows, (h, ?, t), '
                        'filtered by train + valid; prints the line and returns it as the `relation` block.  One GPU.')
    p.add_argument('--classify', action='store_true',
                   help='With --infer: triple classification.  One threshold per relation is fitted on triples-valid.txt '
                        'and the test triples are classified, negatives drawn one per positive by the type-safe sampler '
                        '(draws that are known triples are dropped); prints a line, writes <output_dir>/<model>_classify.json '
                        'and <model>_thresholds.tsv.  One GPU.')
    p.add_argument('--classify_seed', type=int, default=0, help='With --classify: seed of the drawn negatives.')
    p.add_argument('--neighbors', type=int, default=0,
                   help='Write <output_dir>/neighbors.tsv from the checkpoint: the K nearest entities of every entity '
                        'row (no training).  Lines: query, query_name, position, neighbor, neighbor_name, distance.')
    p.add_argument('--neighbors_of', type=str, default=None,
                   help='With --neighbors: a file of entity indices, one per line, to list instead of every entity.')
    p.add_argument('--neighbors_metric', choices=['cosine', 'euclidean'], default='cosine',
                   help='With --neighbors: the distance (cosine: 1 - cos of the rows, as the reference demo ranks).')
    p.add_argument('--min_mentions', type=int, default=50000,
                   help='The minimum number of mentions for an entity to be a viable candidate in inference.')
    # extensions
    p.add_argument('--model', choices=['complex', 'hole'], default='complex')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--max_steps', type=int, default=0, help='Stop after this many steps (0 = epoch limit only).')
    p.add_argument('--checkpoint_seconds', type=float, default=300.,
                   help='Also write the best table found so far this often inside an epoch (0 = once per epoch only).')
    p.add_argument('--optimizer', choices=['sgd', 'adagrad'], default='sgd',
                   help='sgd: the plain gradient descent of holE.py:296; adagrad: AdagradOptimizer in its place (hinge loss, '
                        'one GPU).')
    p.add_argument('--adagrad_init', type=float, default=0.1,
                   help='With --optimizer adagrad: initial_accumulator_value.')
    p.add_argument('--objective', choices=['hinge', 'softmax'], default='hinge',
                   help='hinge: the pairwise ranking loss of holE.py:231 (or --log_loss); softmax: multiclass log-loss of the '
                        'true entity over ALL entities, both sides ("1vsAll"; ComplEx, --optimizer adagrad, one GPU).')
    p.add_argument('--softmax_scale', type=float, default=20.0,
                   help='With --objective softmax: the logit scale (rows are clipped to norm 1, so |score| <= 1).')
    p.add_argument('--softmax_samples', type=int, default=0,
                   help='With --objective softmax: candidates drawn per step from the entity rows (uniform, with '
                        'replacement, shared by the batch and both sides; the true entity has a logit of its own).  '
                        '0: all entity rows, the 1-vs-all objective.')
    p.add_argument('--softmax_labels', choices=['one', 'all'], default='one',
                   help='With --objective softmax (1-vs-all, --softmax_samples 0, --softmax_candidate_sets none): one: a row per '
                        'training triple with its answer as the one label; all: a row per distinct (entity, relation) query '
                        'of each side with ALL its answers among the training triples as labels, the target uniform over '
                        'them (the "KvsAll" training type).')
    p.add_argument('--softmax_candidate_sets', choices=['none', 'types', 'observed'], default='none',
                   help='With --objective softmax (1-vs-all, --softmax_samples 0): each row\'s softmax runs over the candidate '
                        'set of its relation and side -- the sets of --infer --candidate_sets, from train + valid -- instead '
                        'of over all entity rows.')
    p.add_argument('--softmax_validation_ticks', type=int, default=0,
                   help='With --objective softmax: validation ticks per epoch, evenly spaced, the last at the epoch\'s end.  '
                        'Each takes the filtered MRR of --infer (of --infer --candidate_sets with '
                        '--softmax_candidate_sets) over the validation triples on the device and keeps the best table; '
                        'model.ckpt.pt then follows that table.  0: no ticks, the last table is saved.')
    p.add_argument('--softmax_validation_rows', type=int, default=0,
                   help='With --softmax_validation_ticks: rank only this many validation triples, the first of a '
                        'permutation seeded by --seed (0: all of them).')
    p.add_argument('--softmax_patience', type=int, default=0,
                   help='With --softmax_validation_ticks: stop after this many consecutive ticks without an improvement '
                        '(the host then reads every tick).  0: never stop early.')
    p.add_argument('--gpus', type=int, default=1,
                   help='Ranks (one per GPU) the table is row-sharded over; > 1 without a launcher: this program starts them '
                        '(graphembeddings_amd/launch.py).  --batch_size stays the GLOBAL batch.')
    return p


def checkpoint_path(output_dir: str) -> str:
    return os.path.join(output_dir, 'model.ckpt.pt')


def save_checkpoint(output_dir: str, embeddings: torch.Tensor, global_step: int, adagrad_accumulator=None,
                    validation_mrr=None) -> None:
    """adagrad_accumulator (--optimizer adagrad): stored beside the table; without it the file is what it always was.
    validation_mrr (--softmax_validation_ticks): the filtered validation MRR of the tick whose table this is."""
    tmp = checkpoint_path(output_dir) + '.tmp'
    ck = {'embeddings': embeddings.detach().cpu(), 'global_step': int(global_step)}
    if adagrad_accumulator is not None:
        ck['adagrad_accumulator'] = adagrad_accumulator.detach().cpu()
    if validation_mrr is not None:
        ck['validation_mrr'] = float(validation_mrr)
    torch.save(ck, tmp)
    os.replace(tmp, checkpoint_path(output_dir))


def checkpoint_validation_mrr(output_dir: str) -> float:
    """The validation MRR a --softmax_validation_ticks run stored with its best table; 0 when the file holds none."""
    v = torch.load(checkpoint_path(output_dir), weights_only=True).get('validation_mrr')
    return 0.0 if v is None or not v > 0 else float(v)


def load_checkpoint(output_dir: str, device='cuda', with_accumulator: bool = False):
    """(embeddings, global_step); with_accumulator: also the AdaGrad accumulator, None when the file holds none."""
    ck = torch.load(checkpoint_path(output_dir), weights_only=True)
    out = ck['embeddings'].to(device).contiguous(), int(ck['global_step'])
    if not with_accumulator:
        return out
    acc = ck.get('adagrad_accumulator')
    return (*out, None if acc is None else acc.to(device).contiguous())


def check_optimizer_flags(FLAGS, world: int = 1) -> None:
    """--optimizer adagrad: the hinge loss on one GPU."""
    if getattr(FLAGS, 'optimizer', 'sgd') != 'adagrad':
        return
    if FLAGS.log_loss:
        raise SystemExit('--optimizer adagrad is not available with --log_loss (its dense L2 term touches every row)')
    if FLAGS.gpus > 1 or world > 1:
        raise SystemExit('--optimizer adagrad runs on one GPU (drop --gpus)')
    if not FLAGS.adagrad_init > 0:
        raise SystemExit('--adagrad_init must be positive')


def check_objective_flags(FLAGS, world: int = 1) -> None:
    """--objective softmax: ComplEx with AdaGrad on one GPU, no --log_loss; --softmax_samples belongs to it."""
    samples = getattr(FLAGS, 'softmax_samples', 0)
    if samples < 0:
        raise SystemExit('--softmax_samples must not be negative (0: all entity rows)')
    sets = getattr(FLAGS, 'softmax_candidate_sets', 'none') or 'none'
    labels = getattr(FLAGS, 'softmax_labels', 'one') or 'one'
    tick_flags = ('softmax_validation_ticks', 'softmax_validation_rows', 'softmax_patience')
    ticks, rows, patience = (getattr(FLAGS, f, 0) or 0 for f in tick_flags)
    for flag, value in zip(tick_flags, (ticks, rows, patience)):
        if value < 0:
            raise SystemExit('--{} must not be negative'.format(flag))
    if getattr(FLAGS, 'objective', 'hinge') != 'softmax':
        if samples > 0:
            raise SystemExit('--softmax_samples needs --objective softmax')
        if sets != 'none':
            raise SystemExit('--softmax_candidate_sets needs --objective softmax')
        if labels != 'one':
            raise SystemExit('--softmax_labels needs --objective softmax')
        for flag, value in zip(tick_flags, (ticks, rows, patience)):
            if value > 0:
                raise SystemExit('--{} needs --objective softmax (the hinge and log-loss loops have ticks of their '
                                 'own)'.format(flag))
        return
    if sets != 'none' and samples > 0:
        raise SystemExit('--softmax_candidate_sets belongs to the 1-vs-all objective: drop --softmax_samples')
    if labels != 'one' and samples > 0:
        raise SystemExit('--softmax_labels all runs over all entity rows: drop --softmax_samples')
    if labels != 'one' and sets != 'none':
        raise SystemExit('--softmax_labels all runs over all entity rows: drop --softmax_candidate_sets')
    if getattr(FLAGS, 'optimizer', 'sgd') != 'adagrad':
        raise SystemExit('--objective softmax needs --optimizer adagrad')
    if FLAGS.log_loss:
        raise SystemExit('--objective softmax is an objective of its own: drop --log_loss')
    if FLAGS.model != 'complex':
        raise SystemExit('--objective softmax is defined for the ComplEx score (drop --model hole)')
    if FLAGS.gpus > 1 or world > 1:
        raise SystemExit('--objective softmax runs on one GPU (drop --gpus)')
    if not (FLAGS.softmax_scale > 0 and np.isfinite(FLAGS.softmax_scale)):
        raise SystemExit('--softmax_scale must be positive and finite')
    if ticks == 0:
        if rows > 0:
            raise SystemExit('--softmax_validation_rows needs --softmax_validation_ticks')
        if patience > 0:
            raise SystemExit('--softmax_patience needs --softmax_validation_ticks')
    elif sets != 'none' and not H.split_sweep_ok(FLAGS.embedding_dim, 1.0):
        raise SystemExit('--softmax_validation_ticks with --softmax_candidate_sets ranks on the masked sweep: '
                         '--embedding_dim must be a multiple of 8 in 56 ... 288')


def ticks_since_best(mrrs, best: float = 0.0) -> int:
    """How many of the latest ticks in a row did not improve, by the device pocket's rule replayed over the ticks' MRRs in
    order: a tick improves iff its MRR is above the best so far (`best` to start with); a tie keeps the first best, a
    NaN never improves.  What --softmax_patience compares against."""
    since = 0
    for m in mrrs:
        if m > best:
            best, since = m, 0
        else:
            since += 1
    return since


def tick_steps(steps_per_epoch: int, ticks: int) -> set:
    """The steps of an epoch (counted from 1) after which a tick comes: `ticks` of them evenly spaced, the last at the
    epoch's end; fewer where an epoch has fewer steps."""
    return {-(-j * steps_per_epoch // ticks) for j in range(1, ticks + 1)} - {0}


def run_softmax_training(data: D.HolEData, FLAGS, log=print) -> dict:
    """--objective softmax: hole.SoftmaxTrainer over the entity rows relation_count .. entity_count - 1, with the epoch
    and learning-rate bookkeeping of run_training (an epoch is batch_count - 1 steps).  The checkpoint holds the table
    and the AdaGrad accumulator and is written every --checkpoint_seconds, at the end of each epoch and at the end."""
    batch_count = data.triple_count // FLAGS.batch_size
    log('Embedding dimension: ', FLAGS.embedding_dim, 'Batch size: ', FLAGS.batch_size, 'Batch count: ', batch_count)
    if batch_count < 2:
        raise ValueError('need at least 2 batches of training triples')
    if not FLAGS.resume_checkpoint and os.path.isdir(FLAGS.output_dir):
        raise Exception("WARNING: " + FLAGS.output_dir + " already exists!")   # holE.py:254-255
    os.makedirs(FLAGS.output_dir, exist_ok=True)
    global_step, accumulator = 0, None
    if FLAGS.resume_checkpoint:
        embeddings, global_step, accumulator = load_checkpoint(FLAGS.output_dir, with_accumulator=True)
        if tuple(embeddings.shape) != (data.entity_count, FLAGS.embedding_dim):
            raise ValueError('checkpoint shape does not match the data / --embedding_dim')
    else:
        embeddings = H.init_embeddings(data.entity_count, FLAGS.embedding_dim, seed=FLAGS.seed)
    triples = torch.as_tensor(np.ascontiguousarray(data.triples)).cuda()
    candidates = torch.arange(data.relation_count, data.entity_count, dtype=torch.int32, device='cuda')
    kind, candidate_sets = getattr(FLAGS, 'softmax_candidate_sets', 'none') or 'none', None
    if kind != 'none':
        cand = np.arange(data.relation_count, data.entity_count, dtype=np.int32)
        if kind == 'types':
            # candidates of one type next to each other: 64-candidate tiles are then admitted or not as a whole
            cand = cand[np.lexsort((cand, np.asarray(data.type_arrays()[1])[cand]))]
        candidates = torch.as_tensor(np.ascontiguousarray(cand)).cuda()
        _, candidate_sets = E.constrained_sets(data, kind, candidates=cand, device='cuda')
        rel = np.asarray(data.triples)[:, 2]
        log('Softmax candidate sets: {} (from train + valid); mean set size of a training row {:.1f} tails, {:.1f} heads '
            'of {} entity rows'.format(kind, float(candidate_sets['tail'].counts[rel].mean()),
                                       float(candidate_sets['head'].counts[rel].mean()), candidates.numel()))
    trainer = H.SoftmaxTrainer(embeddings, triples, candidates, FLAGS.batch_size, scale=FLAGS.softmax_scale,
                               learning_rate=FLAGS.learning_rate,
                               learning_decay_steps=FLAGS.learning_decay_steps * batch_count,
                               learning_decay_rate=FLAGS.learning_decay_rate, seed=FLAGS.seed,
                               initial_accumulator_value=FLAGS.adagrad_init, n_samples=FLAGS.softmax_samples or None,
                               candidate_sets=candidate_sets, labels=getattr(FLAGS, 'softmax_labels', 'one') or 'one')
    if trainer.labels == 'all':
        log('Softmax labels: all -- {} tail queries and {} head queries (labels from the training triples only) against {} '
            'triples, {} triple sides'.format(len(trainer.queries['tail']), len(trainer.queries['head']),
                                              data.triple_count, 2 * data.triple_count))
    if FLAGS.softmax_samples:
        log('Sampled softmax: {} candidates a step, drawn from the {} entity rows'.format(FLAGS.softmax_samples,
                                                                                      candidates.numel()))
    if accumulator is not None and accumulator.shape == trainer.accumulator.shape:
        trainer.accumulator.copy_(accumulator)
    elif FLAGS.resume_checkpoint:
        log('Checkpoint holds no AdaGrad accumulator: starting it at', FLAGS.adagrad_init)
    trainer.global_step = global_step
    ticks = getattr(FLAGS, 'softmax_validation_ticks', 0) or 0
    patience = getattr(FLAGS, 'softmax_patience', 0) or 0
    # --softmax_validation_ticks: the tick is one native call (evaluate.RankPocket / ge_rank_validation_tick) -- planes,
    # both sides' rank sweeps, the MRR and the pocket copies of the table and the accumulator all happen on the device;
    # the host reads the numbers when it writes the file (after every tick only with --softmax_patience).  What ends up in
    # model.ckpt.pt is the table, accumulator and global step of the best tick, as the hinge loop's write_pocket keeps it.
    vp, best0, at = None, 0.0, set()
    if ticks:
        vp = softmax_rank_pocket(data, FLAGS, embeddings, trainer.accumulator, kind, log)
        if FLAGS.resume_checkpoint:
            best0 = checkpoint_validation_mrr(FLAGS.output_dir)
            vp.best.fill_(best0)
        at = tick_steps(batch_count - 1, ticks)
    else:
        log('Objective softmax: no validation ticks (the hinge tick measures another objective); the mean loss of the last '
            'step is logged per epoch')
    history = []
    state = {'pocket_mrr': best0, 'pocket_step': global_step, 'best_logged': best0, 'last_write': time.time(),
             'stopped': False}

    def drain():
        """Log the ticks since the last call, in order (one synchronisation).  The host sees every MRR in tick order, so it
        knows which tick the device pocket holds: the first one with the highest MRR."""
        for step, m in vp.read():
            log('\tStep {} Validation MRR: {:.6f} (hits@10 {:.2f} %, mean rank {:.1f}, {} rows)...'.format(
                step, m['filtered_mrr'], m['hits10'], m['mean_filtered_pos'], m['counted']))
            history.append((step, m['filtered_mrr']))
            if m['filtered_mrr'] > state['pocket_mrr']:
                state['pocket_mrr'], state['pocket_step'] = m['filtered_mrr'], step

    def write(epoch):
        """Without ticks: the table as it is.  With ticks the file follows the device pocket: once per epoch, every
        --checkpoint_seconds in between, and at the end."""
        state['last_write'] = time.time()
        if vp is None:
            save_checkpoint(FLAGS.output_dir, embeddings, trainer.global_step, trainer.accumulator)
            return
        drain()
        if not state['pocket_mrr'] > state['best_logged']:
            return
        state['best_logged'] = state['pocket_mrr']
        save_checkpoint(FLAGS.output_dir, vp.pocket, state['pocket_step'], vp.pocket_accumulator,
                        validation_mrr=state['pocket_mrr'])
        log('Epoch {}, (Model saved with validation MRR {:.6f})'.format(epoch, state['pocket_mrr']))

    t_start, loss = time.time(), None
    left = FLAGS.max_steps if FLAGS.max_steps else None
    for epoch in range(1, FLAGS.num_epochs + 1):
        log('Training epoch {}...'.format(epoch))
        n = batch_count - 1 if left is None else min(batch_count - 1, left)
        for i in range(1, n + 1):
            loss = trainer.run(1)
            if i in at:
                vp.tick(trainer.global_step)
                if patience:
                    drain()
                    if ticks_since_best([m for _, m in history], best0) >= patience:
                        state['stopped'] = True
                        break
            if FLAGS.checkpoint_seconds > 0 and time.time() - state['last_write'] >= FLAGS.checkpoint_seconds:
                write(epoch)
        write(epoch)
        log('Epoch {}, mean softmax loss {}'.format(epoch, float(loss.mean()) if loss is not None else float('nan')))
        if state['stopped']:
            break
        if left is not None:
            left -= n
            if left <= 0:
                break
    torch.cuda.synchronize()
    if state['stopped']:
        log('Done training -- no improvement in {} validation ticks'.format(patience))
    else:
        log('Done training -- epoch limit reached')
    res = {'steps': trainer.global_step - global_step, 'seconds': time.time() - t_start, 'global_step': trainer.global_step,
           'final_mean_softmax_loss': float(loss.mean()) if loss is not None else float('nan')}
    if vp is not None:
        if not os.path.exists(checkpoint_path(FLAGS.output_dir)):      # no tick improved: the table as it is
            save_checkpoint(FLAGS.output_dir, embeddings, trainer.global_step, trainer.accumulator)
        res.update(pocket_mrr=state['pocket_mrr'], pocket_step=state['pocket_step'], history=history,
                   stopped_early=state['stopped'])
    return res


def softmax_rank_pocket(data: D.HolEData, FLAGS, embeddings: torch.Tensor, accumulator: torch.Tensor, kind: str, log=print):
    """The evaluate.RankPocket of a --softmax_validation_ticks run: the validation triples (the first
    --softmax_validation_rows of a permutation seeded by --seed) ranked over every entity row in id order, filtered by
    train + valid -- the candidates and the filter of --infer -- and, with --softmax_candidate_sets, against the sets of
    --infer --candidate_sets."""
    valid = data.validation_triples
    if valid is None or len(valid) == 0:
        raise ValueError('--softmax_validation_ticks needs validation triples (triples-valid.txt): none found')
    valid = np.asarray(valid, dtype=np.int64)
    rows = getattr(FLAGS, 'softmax_validation_rows', 0) or 0
    if 0 < rows < len(valid):
        valid = valid[np.random.default_rng(FLAGS.seed).permutation(len(valid))[:rows]]
    cand = np.arange(data.relation_count, data.entity_count, dtype=np.int32)
    known = np.concatenate([np.asarray(data.triples), np.asarray(data.validation_triples)], 0)
    sets = None
    if kind != 'none':
        _, sets = E.constrained_sets(data, kind, device='cuda')
    ticks = FLAGS.softmax_validation_ticks
    vp = E.RankPocket(embeddings, valid, cand, known, accumulator=accumulator, candidate_sets=sets,
                      capacity=max(64, 2 * (ticks + 2)))
    log('Objective softmax: {} validation ticks per epoch on the filtered MRR of {} validation triples, both sides{}; '
        'the checkpoint follows the best tick'.format(ticks, len(valid),
                                                      '' if sets is None else ' ({} candidate sets)'.format(kind)))
    return vp


def run_training(data: D.HolEData, FLAGS, log=print) -> dict:
    if getattr(FLAGS, 'objective', 'hinge') == 'softmax':
        check_objective_flags(FLAGS)
        return run_softmax_training(data, FLAGS, log)
    if FLAGS.log_loss and FLAGS.model != 'complex':
        raise NotImplementedError('--log_loss is implemented for the ComplEx score (holE.py:191-196)')
    batch_count = data.triple_count // FLAGS.batch_size
    log('Embedding dimension: ', FLAGS.embedding_dim, 'Batch size: ', FLAGS.batch_size, 'Batch count: ', batch_count)
    if batch_count < 2:
        raise ValueError('need at least 2 batches of training triples')
    if not FLAGS.resume_checkpoint and os.path.isdir(FLAGS.output_dir):
        raise Exception("WARNING: " + FLAGS.output_dir + " already exists!")   # holE.py:254-255
    try:
        os.makedirs(FLAGS.output_dir)
    except OSError as e:
        if e.errno != errno.EEXIST:
            raise
    names, id_to_type, offsets, ids = data.type_arrays()
    tt = H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=FLAGS.padded_size)
    global_step = 0
    adagrad = getattr(FLAGS, 'optimizer', 'sgd') == 'adagrad'
    accumulator = None
    if FLAGS.resume_checkpoint:
        embeddings, global_step, accumulator = load_checkpoint(FLAGS.output_dir, with_accumulator=True)
        if tuple(embeddings.shape) != (data.entity_count, FLAGS.embedding_dim):
            raise ValueError('checkpoint shape does not match the data / --embedding_dim')
    else:
        embeddings = H.init_embeddings(data.entity_count, FLAGS.embedding_dim, seed=FLAGS.seed)
    triples = torch.as_tensor(np.ascontiguousarray(data.triples)).cuda()
    trainer = H.Trainer(embeddings, triples, tt, FLAGS.batch_size, margin=FLAGS.margin,
                        learning_rate=FLAGS.learning_rate,
                        decay_steps=FLAGS.learning_decay_steps * batch_count,
                        decay_rate=FLAGS.learning_decay_rate, model=FLAGS.model, seed=FLAGS.seed,
                        spectral_resident=(FLAGS.model == 'hole' and FLAGS.embedding_dim % 2 == 0 and not FLAGS.log_loss
                                           and not adagrad),
                        optimizer='adagrad' if adagrad else 'sgd',
                        initial_accumulator_value=getattr(FLAGS, 'adagrad_init', 0.1))
    if adagrad and FLAGS.resume_checkpoint:
        if accumulator is not None and accumulator.shape == trainer.accumulator.shape:
            trainer.accumulator.copy_(accumulator)
        else:
            log('Checkpoint holds no AdaGrad accumulator: starting it at', FLAGS.adagrad_init)
    # HolE: `embeddings` is held in the frequency domain while training (hole.Trainer); validation scores it
    # there (model 'hole_spectral'), checkpoints store the real-valued table
    eval_model = 'hole_spectral' if trainer.spectral else FLAGS.model
    trainer.global_step = global_step
    gen = torch.Generator(device='cuda').manual_seed(FLAGS.seed)
    valid = None
    if data.validation_triples is not None and len(data.validation_triples) >= FLAGS.batch_size:
        valid = torch.as_tensor(data.validation_triples).cuda()
    K = max(1, FLAGS.negative_ratio)
    if FLAGS.log_loss:
        # --log_loss (holE.py:206-220): the same native loop, K corrupted batches per step drawn in the prepare launch
        trainer.enable_log_loss(K, FLAGS.l2_regularization)

    # The reference validates 16 times per epoch and keeps the best table ("pocket", holE.py:351-360).  Reading the
    # validation loss on the host at every tick would stop the device every 7 steps at FB15k / B=4096 (and a
    # dozen tensor-op launches per tick cost more host time than the 7 steps take), so the tick is one native call
    # (hole.ValidationPocket / ge_validation_tick): batch selection, negatives, hinge, mean and the pocket copy all
    # happen on the device; the host reads the losses and writes the checkpoint FILE once per epoch.  What ends
    # up in the file is what the reference would have saved: the table and global step of the best tick.
    tick = max(1, batch_count // 16)          # guard for the ZeroDivisionError of holE.py:351
    pocket_loss = 2.
    history = []
    state = {'best_logged': 2.0, 'pocket_step': global_step, 'last_write': time.time()}
    vp = None
    if valid is not None:
        vp = H.ValidationPocket(embeddings, valid, tt, FLAGS.batch_size, margin=FLAGS.margin, model=eval_model,
                                seed=FLAGS.seed ^ 0x5EED, capacity=max(64, 2 * (batch_count // tick + 2)),
                                log_loss=(K, FLAGS.l2_regularization) if FLAGS.log_loss else None)

    def validation_tick():
        vp.tick(trainer.global_step, trainer.global_step)

    def drain():
        """Log the validation ticks since the last call, in order (one synchronisation).  The host sees every loss
        in tick order, so it knows which tick the device pocket holds: the first one with the lowest loss."""
        nonlocal pocket_loss
        ticks = vp.read() if vp is not None else []
        for step, vlm in ticks:
            log('\tStep {} Validation Loss: {}...'.format(step, vlm))
            history.append((step, vlm))
            if vlm < pocket_loss:
                pocket_loss = vlm
                state['pocket_step'] = step

    def write_pocket(epoch):
        """The checkpoint file follows the device pocket: once per epoch, every --checkpoint_seconds in between (the
        reference saves at every improving tick, holE.py:357-360: a killed run loses at most that much), and at the end."""
        drain()
        state['last_write'] = time.time()
        pocket = vp.pocket if vp is not None else None
        if pocket is None or pocket_loss >= state['best_logged']:
            return
        state['best_logged'] = pocket_loss
        table = pocket.clone()
        if trainer.spectral:
            H.hole_from_spectral(table)
        save_checkpoint(FLAGS.output_dir, table, state['pocket_step'], trainer.accumulator)
        log('Epoch {}, (Model saved with loss {})'.format(epoch, pocket_loss))

    t_start = time.time()
    done = False
    epoch = 0
    for epoch in range(1, FLAGS.num_epochs + 1):
        log('Training epoch {}...'.format(epoch))
        trainer.reshuffle(gen)
        if epoch < FLAGS.num_epochs:
            trainer.prepare_reshuffle(gen)        # the next epoch's order is drawn beside this epoch's steps
        batch = 1
        while batch < batch_count and not done:
            if batch % tick == 0 and valid is not None:
                validation_tick()
            # steps up to the next validation tick (or the end of the epoch), enqueued natively
            nxt = min(batch_count, (batch // tick + 1) * tick)
            n = nxt - batch
            if FLAGS.max_steps:
                n = min(n, FLAGS.max_steps - (trainer.global_step - global_step))
            if n > 0:
                trainer.run(n)
            if FLAGS.checkpoint_seconds > 0 and time.time() - state['last_write'] >= FLAGS.checkpoint_seconds:
                write_pocket(epoch)
            batch += max(n, 0)
            if FLAGS.max_steps and trainer.global_step - global_step >= FLAGS.max_steps:
                done = True
            if n <= 0:
                break
        write_pocket(epoch)
        if done:
            break
    torch.cuda.synchronize()
    log('Done training -- epoch limit reached')
    trainer.to_real()
    if not os.path.exists(checkpoint_path(FLAGS.output_dir)):
        save_checkpoint(FLAGS.output_dir, embeddings, trainer.global_step, trainer.accumulator)
    steps = trainer.global_step - global_step
    return {'steps': steps, 'seconds': time.time() - t_start, 'pocket_loss': pocket_loss, 'history': history,
            'global_step': trainer.global_step, 'final_mean_hinge': float(trainer.last_loss.mean())}


def save_embeddings(FLAGS, log=print):
    """holE.py:501-527: print every row's complex embedding (clipped, as get_embedding returns it)."""
    data = D.init_inference_data(FLAGS.data_dir, min_mentions=None)
    emb, _ = load_checkpoint(FLAGS.output_dir)
    k = emb.shape[1] // 2
    norm = emb.norm(dim=1, keepdim=True).clamp_min(1.0)
    y = (emb / norm).cpu().numpy()
    for entity in range(data.entity_count):
        log(data.id_to_metadata.get(entity, str(entity)), y[entity, :k] + 1j * y[entity, k:])


def infer_triples(FLAGS, log=print) -> dict:
    """--infer: the ranking / MRR semantics of holE.py:427-490 as a filtered 1-vs-all link-prediction
    evaluation over every entity row (the reference's candidate lists are Diffbot-specific,
    holE.py:534-541)."""
    data = D.init_inference_data(FLAGS.data_dir, min_mentions=None)
    emb, _ = load_checkpoint(FLAGS.output_dir)
    # --model hole: the checkpoint holds the real-valued table; ranks use the HolE score (README.md:42), not ComplEx
    # positions are recorded for confident sweeps only: lowest loss < --infer_threshold (holE.py:436-438, 464-466, 616)
    out = E.evaluate_fb15k_style(emb, data, both_sides=True, model=FLAGS.model, infer_threshold=FLAGS.infer_threshold)
    tail_sets = None
    if getattr(FLAGS, 'candidate_sets', None):
        # the type-constrained protocol: the sets come from train + valid, every test row is recorded (no gate)
        out['constrained'], sets = E.evaluate_constrained(emb, data, FLAGS.candidate_sets, model=FLAGS.model)
        tail_sets = sets['tail']
    if FLAGS.predict_k > 0:
        # the reference's prediction lines (holE.py:445-456), into the output directory (truncated), not appended to ./
        E.predict_inference_results(emb, data, FLAGS.predict_k, FLAGS.infer_threshold,
                                    os.path.join(FLAGS.output_dir, 'inference_results.tsv'), model=FLAGS.model, log=log,
                                    candidate_sets=tail_sets)
    if getattr(FLAGS, 'relation_ranks', False):
        # (h, ?, t): the head-side sweep over the relation rows on the triples with head and relation exchanged
        parts = [a for a in (data.triples, data.validation_triples) if a is not None]
        raw, fil = E.relation_ranks(emb, data.test_array, data.relation_count, np.concatenate(parts, 0) if parts else None,
                                    model=FLAGS.model)
        out['relation'] = rel = E.mrr_and_hits(raw, fil)
        log('relation: raw MRR {raw_mrr:.6f} (mean rank {mean_raw_pos:.1f}); filtered MRR {filtered_mrr:.6f} '
            '(mean rank {mean_filtered_pos:.1f}); hits@1/3/10 {hits1:.2f} / {hits3:.2f} / {hits10:.2f} %'.format(**rel))
    if getattr(FLAGS, 'classify', False):
        out['classify'] = classify_triples(FLAGS, data, emb, log=log)
    return out


def classify_triples(FLAGS, data, emb, log=print) -> dict:
    """--infer --classify: thresholds fitted on the validation split, the test split classified, negatives from the
    type-safe sampler filtered by train + valid + test; <model>_classify.json and <model>_thresholds.tsv."""
    from . import classify as C
    if data.validation_triples is None or len(data.validation_triples) == 0:
        raise SystemExit('--classify needs triples-valid.txt')
    _, id_to_type, offsets, ids = data.type_arrays()
    tt = H.TypeTables.from_host(id_to_type, offsets, ids, padded_size=FLAGS.padded_size)
    known = np.concatenate([a for a in (data.triples, data.validation_triples, data.test_array) if a is not None], 0)
    res = C.triple_classification(C.TableModel(emb, data.relation_count, tt, FLAGS.model), data.validation_triples,
                                  data.test_array, known=known, seed=FLAGS.classify_seed)
    log(C.summary_line(res))
    json_path = os.path.join(FLAGS.output_dir, f'{FLAGS.model}_classify.json')
    tsv = os.path.join(FLAGS.output_dir, f'{FLAGS.model}_thresholds.tsv')
    C.write_results(res, json_path, tsv)
    log(f'wrote {json_path} and {tsv}')
    return C.report(res)


def check_classify_flags(FLAGS, world: int = 1) -> None:
    """--classify is part of --infer, on one GPU."""
    if not FLAGS.classify:
        return
    if not FLAGS.infer:
        raise SystemExit('--classify needs --infer')
    if FLAGS.gpus > 1 or world > 1:
        raise SystemExit('--classify runs on one GPU (drop --gpus)')
    if FLAGS.classify_seed < 0:
        raise SystemExit('--classify_seed must be >= 0')


def check_candidate_set_flags(FLAGS, world: int = 1) -> None:
    """--candidate_sets is part of --infer, on one GPU."""
    if not getattr(FLAGS, 'candidate_sets', None):
        return
    if not FLAGS.infer:
        raise SystemExit('--candidate_sets needs --infer')
    if FLAGS.gpus > 1 or world > 1:
        raise SystemExit('--candidate_sets runs on one GPU (drop --gpus)')


def check_neighbor_flags(FLAGS, world: int = 1) -> None:
    """--neighbors is a mode of its own, on one GPU, like --save_embeddings: refused with training-only or other modes."""
    if FLAGS.neighbors < 0:
        raise SystemExit('--neighbors must be >= 0')
    if not FLAGS.neighbors:
        if FLAGS.neighbors_of is not None:
            raise SystemExit('--neighbors_of needs --neighbors K')
        return
    if FLAGS.gpus > 1 or world > 1:
        raise SystemExit('--neighbors runs on one GPU (drop --gpus)')
    if FLAGS.infer or FLAGS.save_embeddings:
        raise SystemExit('--neighbors is a mode of its own: drop --infer / --save_embeddings')
    if FLAGS.neighbors_of is not None and not os.path.isfile(FLAGS.neighbors_of):
        raise SystemExit(f'--neighbors_of: no such file: {FLAGS.neighbors_of}')


def read_neighbors_of(path: str, entity_count: int) -> np.ndarray:
    """The entity indices of a --neighbors_of file, one per line (blank lines skipped), checked against the table."""
    ids = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            try:
                ids.append(int(line))
            except ValueError:
                raise SystemExit(f'{path}:{n}: not an entity index: {line!r}')
    a = np.asarray(ids, dtype=np.int64)
    if a.size and (a.min() < 0 or a.max() >= entity_count):
        raise SystemExit(f'{path}: entity indices must lie in [0, {entity_count})')
    return a


def write_neighbors(FLAGS, log=print) -> int:
    """--neighbors K: the K nearest entity rows of every entity row (or of --neighbors_of's) by --neighbors_metric, over
    the checkpoint's table as stored, into <output_dir>/neighbors.tsv.  Candidates: the entity rows
    [relation_count, entity_count); a query's own row is not its neighbour."""
    from . import neighbors as NB
    data = D.init_inference_data(FLAGS.data_dir, min_mentions=None)
    emb, _ = load_checkpoint(FLAGS.output_dir)
    R, E = data.relation_count, data.entity_count
    queries = np.arange(R, E) if FLAGS.neighbors_of is None else read_neighbors_of(FLAGS.neighbors_of, E)
    path = os.path.join(FLAGS.output_dir, 'neighbors.tsv')
    n = NB.write_neighbors(path, emb.contiguous(), queries, FLAGS.neighbors, candidates=np.arange(R, E),
                           metric=FLAGS.neighbors_metric, names=data.id_to_metadata)
    log(f'wrote {path} ({n} lines)')
    return n


def main(argv=None):
    FLAGS, _unparsed = build_parser().parse_known_args(argv)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    check_neighbor_flags(FLAGS, world)
    if FLAGS.neighbors:
        write_neighbors(FLAGS)
        return
    if FLAGS.predict_k < 0:
        raise SystemExit('--predict_k must be >= 0')
    if FLAGS.predict_k and (FLAGS.gpus > 1 or world > 1):
        raise SystemExit('--predict_k runs on one GPU: top-k prediction over a row-sharded table is not implemented '
                         '(drop --gpus or --predict_k)')
    check_classify_flags(FLAGS, world)
    check_candidate_set_flags(FLAGS, world)
    check_optimizer_flags(FLAGS, world)
    check_objective_flags(FLAGS, world)
    if FLAGS.relation_ranks and not FLAGS.infer:
        raise SystemExit('--relation_ranks needs --infer')
    if FLAGS.relation_ranks and (FLAGS.gpus > 1 or world > 1):
        raise SystemExit('--relation_ranks runs on one GPU (drop --gpus)')
    if FLAGS.gpus > 1 and 'WORLD_SIZE' not in os.environ and not FLAGS.save_embeddings:
        # no launcher: this process (which has not touched the GPU) becomes the parent of --gpus ranks of itself
        from . import launch
        sys.exit(launch.spawn_ranks(FLAGS.gpus, list(sys.argv[1:] if argv is None else argv), module='graphembeddings_amd.train'))
    if world > 1 and FLAGS.gpus != world:
        raise SystemExit(f'--gpus {FLAGS.gpus} but the launcher started {world} ranks')
    if world > 1 and not FLAGS.save_embeddings:
        from . import sharded_train as ST
        if FLAGS.infer:
            ST.infer_sharded(FLAGS)
        else:
            training_data = D.init_data(FLAGS.data_dir, cache=True)
            if int(os.environ.get('RANK', '0')) == 0:
                print('Entities: ', training_data.entity_count - training_data.relation_count, 'Relations: ',
                      training_data.relation_count, 'Triples: ', training_data.triple_count)
            ST.run_training_sharded(training_data, FLAGS)
        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()
        return
    if FLAGS.save_embeddings:
        save_embeddings(FLAGS)
    elif FLAGS.infer:
        infer_triples(FLAGS)
    else:
        training_data = D.init_data(FLAGS.data_dir, cache=True)
        print('Entities: ', training_data.entity_count - training_data.relation_count, 'Relations: ',
              training_data.relation_count, 'Triples: ', training_data.triple_count)
        run_training(training_data, FLAGS)


if __name__ == '__main__':
    main(sys.argv[1:])
