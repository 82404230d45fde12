"""examples/embedding_offload.py --bags on CPU daemons: the pooled lookup on the host path against
torch.nn.functional.embedding_bag, within the bound the example derives."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_embedding_example_bags_cpu(native):
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "embedding_offload.py"), "--rows", "3000", "--bags", "64"],
                       capture_output=True, text=True, timeout=300, cwd="/tmp", env=dict(os.environ, OCM_NO_GPU="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "lookups equal index_select" in r.stdout and "--bags: 64 bags" in r.stdout and "'n_bag': 3" in r.stdout
