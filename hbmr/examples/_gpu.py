"""The ``-gpu`` path the example drivers share."""
from __future__ import annotations

from ..mapred import JobConf


def run_gpu_job(build, classic_name, conf, cluster, log):
    """Run the split-level job ``build()`` returns: on ``cluster``, or on a
    LocalCluster over this host's GPUs made for the run.  Returns the
    RunningJob, or None when ``build`` raised ValueError (not eligible: ``log``
    gets the reason and the caller runs the classic ``classic_name`` job).
    Raises RuntimeError if the job fails."""
    try:
        job = build()
    except ValueError as e:
        log.warning("%s; running the classic %s job", e, classic_name)
        return None
    own = cluster is None
    if own:
        import torch
        from ..mapred.cluster import LocalCluster
        gpus = [list(range(torch.cuda.device_count()))] if torch.cuda.is_available() else None
        cluster = LocalCluster(JobConf(conf), num_trackers=1, gpus=gpus)
    try:
        rj = cluster.submit_job(job)
        rj.waitForCompletion()
        if not rj.isSuccessful():
            raise RuntimeError(f"Job failed: {rj.getID()} {rj.getFailureInfo()}")
    finally:
        if own:
            cluster.shutdown()
    return rj
