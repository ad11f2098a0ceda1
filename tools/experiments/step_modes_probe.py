"""Where do two runs of the bench-shape training loop part?  25 steps in this process (the loop bench.py times: reference_loss, flat
clip, fused Adam); per step one line with the md5 of what the step computed -- temporal scores, the three losses, logits, the clipped
flat gradient, the proposal count -- taken from device copies after the last step, so the steps run unobserved.

  for i in 1 2 3 4 5 6 7; do python tools/experiments/step_modes_probe.py > run_$i.log; done; md5sum run_*.log
  STAGE_STREAMS=0 python tools/experiments/step_modes_probe.py

Finding 70: with the default branch streams the 25-step trajectory has TWO outcomes from process to process (3 of 7 / 4 of 7 here),
parting in the gradient of step 20 after a bit-equal forward, while the proposal count changes from step to step; with
STAGE_STREAMS=0 seven of seven processes agree.  Optional argument: the root of another tree to import the package from."""
import contextlib, hashlib, os, sys, gc
root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
import torch
from tvqaplus_amd import parallel
from tvqaplus_amd.stage import STAGE, reference_loss
from tvqaplus_amd.synth import make_batch, make_opt
dev = torch.device("cuda:0")
torch.manual_seed(2018)
opt = make_opt(hsz=128, add_local=True, dropout=0.1, use_sup_att=True, input_encoder_n_heads=0, cls_encoder_n_heads=0, storage_dtype="fp32")
with contextlib.redirect_stdout(open(os.devnull, "w")):
    model = STAGE(opt).to(dev).train()
batch = make_batch(N=16, Li=300, Lr=20, Lw=50, Lqa=40, seed=2018, ragged=True, att_imgs=4, att_words=3).to(dev)
params = [p for p in model.parameters() if p.requires_grad]
bucket = parallel.FlatGradBucket(params)
optimizer = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-7, fused=True)
rec = []
gc.collect()
for step in range(25):
    if step == 5:
        gc.freeze()
    bucket.zero()
    (out, targets), att_loss, _, t_loss, t_scores = model(batch)
    loss = reference_loss(out, targets, att_loss, t_loss, 16, 0.1, 0.5, scale=16.0 / len(targets))
    loss.backward()
    bucket.all_reduce()
    bucket.clip_grad_norm_(10.0)
    g = bucket.flat.clone()
    optimizer.step()
    rec.append(dict(t_scores=t_scores.detach().clone(), att=att_loss.detach().clone(), ts=t_loss.detach().clone(), logits=out.detach().clone(),
                    loss=loss.detach().clone(), grad=g, P=torch.tensor(len(targets))))
torch.cuda.synchronize()
for s, r in enumerate(rec):
    print("STEP %02d " % s + " ".join("%s=%s" % (k, hashlib.md5(v.cpu().numpy().tobytes()).hexdigest()[:6]) for k, v in r.items()))
