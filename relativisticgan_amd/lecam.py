"""LeCam regularisation of D (--rgan_lecam; Tseng et al., "Regularizing GANs under limited data",
CVPR 2021): the anchors -- moving averages of D's outputs on the real and on the generated batch
-- and the hyper-parameters of the term, kept on the device.  The term itself, its gradients and
the move of the anchors are one HIP launch per D step (csrc/lecam.hip, losses.lecam); DESIGN.md
§7.2 has the definition."""
import torch


class LeCam:
    """Two device arrays, ``state`` = double[4] {a_real, a_fake, calls, 0} and ``hyper`` =
    double[4] {lambda, beta, start, 0} (include/rgan.h rgan_lecam).  The kernel reads both at run
    time and nothing on the host, so an iteration captured in a HIP graph keeps moving the
    anchors across replays and follows a hyper-parameter written between them.  Under data
    parallelism every rank holds the same state: the anchors move on all-reduced sums."""

    def __init__(self, device, lam, beta=0.99, start=1):
        self.state = torch.zeros(4, dtype=torch.float64).to(device)
        self.hyper = torch.tensor([float(lam), float(beta), float(start), 0.0], dtype=torch.float64).to(device)

    def restart(self):
        """Nothing averaged yet: the next D step initialises the anchors with its batch means."""
        with torch.no_grad():
            self.state.zero_()

    def read(self):
        """(a_real, a_fake): one small device read."""
        a_real, a_fake, _, _ = self.state.tolist()
        return a_real, a_fake

    def state_dict(self):
        """No collective: the ranks agree."""
        a_real, a_fake, calls, _ = self.state.tolist()
        return {"a_real": a_real, "a_fake": a_fake, "calls": calls}

    def load_state_dict(self, sd):
        with torch.no_grad():
            self.state.copy_(torch.tensor([float(sd["a_real"]), float(sd["a_fake"]), float(sd["calls"]), 0.0],
                                          dtype=torch.float64))
