"""Evaluators of the reference's ldm/notebook_utils.py: Experiment_Colab (:28-39, EMA parameters of a checkpoint),
the variational-bound BPD evaluators (:157-191), the exact-likelihood ODE evaluator (:232-373, 446-531) and the views of
the learned noise schedule (:554-711); bound_profile / plot_bound_profile (not in the reference) take the bound apart;
nearest_neighbours / sample_novelty / precision_recall / plot_neighbours (not in the reference) ask whether samples are new;
dct2 (:730-733, there on skimage and scipy) and image_spectrum / compare_spectra / schedule_spectrum / plot_spectra (not
in the reference) look at spatial frequency; image_fidelity / restoration_quality / diversity / plot_fidelity (not in the
reference) give the PSNR and SSIM of restorations against their originals; pca_transformation,
plot_tsne_transformation and animate_scatter (:713-753, there on sklearn; here exact t-SNE on the device) and tsne / latent_map (not in the reference) look at the latent space;
set_moments / frechet_distance / compare_moments / eigen_images / plot_eigen_images (not in the reference) give the
pixel-space Frechet distance of two image sets from their exact moments."""
from mulan_amd.evaluators import (Experiment_Colab, Hutchinson, eval_bpd_dense_sampling,  # noqa: F401
                                  eval_bpd_ode, eval_bpd_sparse_sampling, get_ode_likelihood_fn, get_logits, get_sample_fn,
                                  logits_to_embeddings, _get_bpd_offset)
from mulan_amd.evaluators import (Clustering, get_embedding, heat_map_panels, noise_schedule_per_embedding,  # noqa: F401
                                  noise_schedule_summary, plot_heat_map, plot_histogram, plot_noise_schedule)
from mulan_amd.evaluators import bound_profile, plot_bound_profile  # noqa: F401
from mulan_amd.neighbours import nearest as nearest_neighbours, novelty as sample_novelty  # noqa: F401
from mulan_amd.neighbours import precision_recall, plot_neighbours  # noqa: F401
from mulan_amd.spectrum import (compare_spectra, dct2, image_spectrum, plot_spectra,  # noqa: F401
                                schedule_spectrum)
from mulan_amd.fidelity import (diversity, image_fidelity, plot_fidelity, psnr_from_sse,  # noqa: F401
                                restoration_quality)
from mulan_amd.latent_maps import (animate_scatter, latent_map, pca_transformation,  # noqa: F401
                                   plot_tsne_transformation, tsne)
from mulan_amd.moments import (compare_moments, eigen_images, frechet_distance,  # noqa: F401
                               plot_eigen_images, set_moments)
