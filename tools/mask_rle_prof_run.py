"""rocprofv3 target for the two device RLE string kernels (csrc/mask_rle.hip) alone:

    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/mask_rle_prof_run.py paths
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/mask_rle_prof_run.py predict [N]

paths:   instances.nms_encode on 100 noisy 480 x 640 masks, 20 calls by the chain (mask_runs_count / emit + mask_rle_kernel) and 20 by
         the fused kernel — predict() itself takes the fused path at every width up to 1024, so the chain needs a driver of its own;
predict: tools/instance_bench.py's set-up (B = 8, 336 x 336, random-weight outputs) with N (default 40) instance predicts instead of
         its three.  ZUTIS_HIP_LIB names the library under test (profiles/NOTES.md, "COCO RLE: one codec")."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "zutis_amd", "dropin"))
import numpy as np, torch                                                                                          # noqa: E401,E402
from zutis_amd import detgen, instances                                                                             # noqa: E402

dev = torch.device("cuda:0")
mode = sys.argv[1] if len(sys.argv) > 1 else "paths"
if mode == "paths":
    rng = np.random.default_rng(3)
    B, Q, H, W = 1, 100, 480, 640
    masks = np.zeros((B, Q, H, W), np.uint8)
    for q in range(Q):
        y0, x0 = rng.integers(0, H - 200), rng.integers(0, W - 300)
        blob = rng.random((rng.integers(60, 200), rng.integers(80, 300))) > 0.05      # noisy blobs: a thousand transitions and more
        masks[0, q, y0:y0 + blob.shape[0], x0:x0 + blob.shape[1]] = blob
    scores = (rng.random((B, Q)) * 0.9 + 0.05).astype(np.float32)
    cats = rng.integers(1, 40, (B, Q)).astype(np.int64)
    md, sd, cd = torch.from_numpy(masks).to(dev), torch.from_numpy(scores).to(dev), torch.from_numpy(cats).to(dev)
    for fused in (False, True):
        for _ in range(20):
            r = instances.nms_encode(md, sd, cd, "hard", fused=fused)
        print(f"fused={fused}: {len(r.kept)} kept, {sum(len(x['counts']) for x in r.rles) / max(1, len(r.rles)):.0f} characters per string")
else:
    from networks.zutis import ZUTIS
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    net = ZUTIS(categories=[f"c{i}" for i in range(81)], device=dev, text_embeddings=torch.from_numpy(detgen.text_embeddings(81, 512)))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in detgen.zutis_state_dict(detgen.VIT_B16).items()}, strict=True)
    net = net.to(dev).eval()
    with torch.no_grad():
        out = net(torch.from_numpy(detgen.images(8, 336, 336)).to(dev))
        for _ in range(n):
            preds = net.predict(out, mask_type="instance", size=(336, 336), nms_type="hard")
    print(f"{n} predicts, {len(preds)} predictions each")
torch.cuda.synchronize()
