"""Best-of-N behind ZbufferModelPts.get_best_sample (z_buffermodel.py): what decides the route and the scope of the ranking, the
candidates of a view as one lazy sequence of decoded images, and one ranker per route -- the host's, the device's for one view, the
device's per view -- with one ending for candidates dealt over the ranks.  The device passes themselves are ranking.py's."""
import itertools
import os

import numpy as np
import torch

from . import distributed as D
from . import ranking
from .lmconv.model import wavefronts


def rank_samples(discrim_scores, entropy_scores):
    """Index of the sample get_best_sample keeps (z_buffermodel.py:266-276): samples are ranked by discriminator score
    (ascending) and by classifier entropy (ascending); total = .5*(n-1-entropy_rank) + .5*discrim_rank; the first
    arg-max wins.  Ranks come from numpy's default argsort, as there."""
    n = len(discrim_scores)
    by_disc, by_entr = np.argsort(np.asarray(discrim_scores)), np.argsort(np.asarray(entropy_scores))
    disc_rank, entr_rank = np.empty(n, np.int64), np.empty(n, np.int64)
    disc_rank[by_disc] = np.arange(n)
    entr_rank[by_entr] = np.arange(n)
    return int(np.argmax(.5 * (n - 1 - entr_rank) + .5 * disc_rank))


def resolve_option(arg, opt, name, env, allowed, default):
    """The value of get_best_sample's argument `name` in effect: the argument, else opt.<name>, else the environment variable `env`,
    else `default` (None: nothing was asked for).  The variable is read per call -- which is why networks/routing.Switch, whose
    process default is a module global filled at import, is not the tool here.  ValueError for a value outside `allowed`."""
    value = arg if arg is not None else getattr(opt, name, None)
    if value is None:
        value = os.environ.get(env, default)
    if value is not None and value not in allowed:
        raise ValueError(f"get_best_sample: {name} / opt.{name} / {env} is {value!r}, expected one of {allowed}")
    return value


RANK_ROUTES = ("host", "device")


def _rank_route(rank_on, opt):
    """rank_on of get_best_sample -> "host" / "device"; None: opt.rank_on, then the environment variable PS_RANK (read per call), host
    by default"""
    return resolve_option(rank_on, opt, "rank_on", "PS_RANK", RANK_ROUTES, "host")


RANK_SCOPES = ("batch", "view")


def _rank_scope(rank_scope, opt):
    """rank_scope of get_best_sample -> "batch" (one winner index for the whole batch: the reference's rule) / "view" (the best
    candidate of every view); None: opt.rank_scope, then the environment variable PS_RANK_SCOPE (read per call), batch by default"""
    return resolve_option(rank_scope, opt, "rank_scope", "PS_RANK_SCOPE", RANK_SCOPES, "batch")


def view_draws(n, B, L):
    """(n, B, L) uniforms on the host for n candidates of B views: entry [i, b] is the (1, L) draw of manual_seed(i) for every b -- a
    view gets the draws of a B = 1 run, never row b of a (B, L) draw: it is the same picture alone or in a batch"""
    return torch.stack([torch.rand(1, L, generator=torch.Generator(device="cpu").manual_seed(i)).expand(B, L) for i in range(n)])


def candidates(model, plan, codes, background_mask, gen_fs, uniforms, which):
    """The candidates `which` (indices into uniforms (num_samples,B,L)) of the B views of `codes`, outpainted and decoded -> (i, img
    (B,3,S,S)) in the order of `which`.  A generator: candidate i + 1 is decoded when the caller asks for it, so the host route has
    scored candidate i by then.
    The candidates are independent AR runs of the same view(s): they go through the sampler TOGETHER, as k * B frames
    (sample-major) that share the view's order and masks and differ in their draws -- one wavefront schedule, the
    launches of one run instead of k runs one after the other (the num_samples candidates are one of
    the path's natural parallel axes)."""
    B, G = codes.shape[0], model.obs[1]
    L = G * model.obs[2]
    per = max(1, min(len(which), model.sample_batch // max(B, 1)))          # candidates per engine run
    for s0 in range(0, len(which), per):
        idx = which[s0:s0 + per]
        k = len(idx)
        rep = lambda t: t.repeat((k,) + (1,) * (t.dim() - 1)).contiguous()
        waves = plan.waves
        if k > 1:
            waves = wavefronts(np.tile(plan.order_host, (k, 1)), G, model.obs[2], plan.first_step, codes.device)
        c = rep(codes.reshape(B, L).to(torch.int32))
        eng = model._engine(k * B)
        eng.ar_run(c, rep(plan.order_loc), rep(plan.region), rep(plan.mask_init), rep(plan.mask_undilated),
                   rep(plan.mask_dilated), temperature=model.opt.temperature,
                   uniforms=uniforms[idx].reshape(k * B, L).contiguous(), first_step=plan.first_step, waves=waves)
        eng.check()
        for j, i in enumerate(idx):
            yield i, model._decode_checked(gen_fs, background_mask, c[j * B:(j + 1) * B].view(B, G, model.obs[2]))


def peek(cands):
    """-> (the first candidate's image, or None where there is none; the same candidates, the first included, as lazy as before)"""
    first = next(cands, None)
    return (None, cands) if first is None else (first[1], itertools.chain((first,), cands))


def sharded_winner(imgs, disc, entr, n, world, device):
    """The ending for candidates dealt over the ranks: imgs {i: img} and the scores of this rank's own; two scalars per candidate are
    gathered, every rank applies the rank rule and the owner of the winner broadcasts it (a rank without candidates learns the
    shape from the owner)"""
    d_all, e_all = D.gather_scores(disc, entr, n)
    best = rank_samples(list(d_all), list(e_all))
    return D.broadcast_from(imgs.get(best), D.owner_of(best, world), device)


def rank_on_host(model, cands, netD, input_img, n, world, device):
    """The reference's route: every candidate is scored as it is decoded, one at a time through the host -> the winner's image"""
    imgs, disc, entr = {}, [], []
    for i, img in cands:
        imgs[i] = img
        disc.append(float(netD.run_discriminator_one_step(img, input_img)["D_Fake"].mean().cpu()))
        entr.append(model._entropy_score(img))
    if len(imgs) < n:
        return sharded_winner(imgs, disc, entr, n, world, device)
    return imgs[rank_samples(disc, entr)]


def rank_on_device(model, cands, netD, n, world, device):
    """B = 1: the candidates are stacked and scored in one batch where they are, the rank rule runs there too and the winner comes back
    through index_select -- no score comes down (candidates dealt over the ranks: the two vectors of this rank's own, once)"""
    imgs = dict(cands)
    stack = torch.cat(list(imgs.values()))
    disc_dev, entr_dev = ranking.score_candidates(stack, netD, model.classifier)
    if len(imgs) == n:
        return stack.index_select(0, ranking.select(disc_dev, entr_dev))
    disc, entr = torch.stack([disc_dev, entr_dev]).double().cpu().tolist()    # the one download of this rank's scores
    return sharded_winner(imgs, disc, entr, n, world, device)


def rank_per_view(model, cands, netD, n, B):
    """B > 1 views, each keeps the best of ITS n candidates -> (B,3,S,S); no score and no index comes down"""
    stack = torch.cat([img for _, img in cands])          # candidate-major: candidate i of view b at i * B + b
    if not ranking.can_score_on_device(netD, model.classifier, stack):
        raise NotImplementedError(f"get_best_sample: num_samples = {n} with rank_scope='view': ranking.can_score_on_device does "
                                  f"not take candidates of shape {tuple(stack.shape)} {stack.dtype}")
    chunk = getattr(model.opt, "rank_chunk", None) or ranking.SCORE_CHUNK      # (a cap on the scorers' memory)
    disc_dev, entr_dev = ranking.score_candidates(stack, netD, model.classifier, chunk)
    return ranking.take_groups(stack, ranking.select_groups(disc_dev, entr_dev, B, n), n)
