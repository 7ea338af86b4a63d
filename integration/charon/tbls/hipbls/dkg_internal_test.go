//go:build hipbls

package hipbls

import (
	"math/big"
	"testing"

	promtest "github.com/prometheus/client_golang/prometheus/testutil"
	"github.com/stretchr/testify/require"

	"github.com/obolnetwork/charon/tbls"
)

// sumModOrder is the sum of the scalars mod the group order, as 32 big-endian bytes.
func sumModOrder(keys ...tbls.PrivateKey) tbls.PrivateKey {
	acc := new(big.Int)
	for _, k := range keys {
		acc.Add(acc, new(big.Int).SetBytes(k[:]))
	}
	acc.Mod(acc, order)
	var out tbls.PrivateKey
	acc.FillBytes(out[:])

	return out
}

// TestDealWithCommitmentsEqualsHerumi: the shares of every validator dealt in one call recover the secret under
// tbls.Herumi{}'s RecoverSecret, commitment 0 is tbls.Herumi{}'s SecretToPublicKey of the secret, and the commitments
// evaluated at each operator index give tbls.Herumi{}'s SecretToPublicKey of that share; a secret that does not
// deserialize fails alone; the metrics advance under "deal_commit".
func TestDealWithCommitmentsEqualsHerumi(t *testing.T) {
	h, err := New()
	require.NoError(t, err)
	ref := tbls.Herumi{}
	const n, total, threshold = 5, 4, 3
	secrets := make([]tbls.PrivateKey, n)
	for i := range secrets {
		secrets[i], err = ref.GenerateSecretKey()
		require.NoError(t, err)
	}
	for i := range secrets[2] {
		secrets[2][i] = 0xff // above r
	}

	items := func(path string) float64 { return promtest.ToFloat64(itemsCounter.WithLabelValues(path)) }
	failed := func(path string) float64 { return promtest.ToFloat64(failedCounter.WithLabelValues(path)) }
	i0, f0 := items("deal_commit"), failed("deal_commit")
	dealt, errs, err := h.DealWithCommitments(secrets, total, threshold)
	require.NoError(t, err)
	require.Len(t, dealt, n)
	require.InDelta(t, n, items("deal_commit")-i0, 0)
	require.InDelta(t, 1, failed("deal_commit")-f0, 0)

	var polys [][][]tbls.PublicKey
	var good []int
	for v, d := range dealt {
		if v == 2 {
			require.ErrorContains(t, errs[v], "cannot unmarshal bytes into Herumi secret key")

			continue
		}
		require.NoError(t, errs[v])
		require.Len(t, d.Shares, total)
		require.Len(t, d.Commitments, threshold)
		pk, err := ref.SecretToPublicKey(secrets[v])
		require.NoError(t, err)
		require.Equal(t, pk, d.Commitments[0])
		back, err := ref.RecoverSecret(map[int]tbls.PrivateKey{1: d.Shares[1], 3: d.Shares[3], 4: d.Shares[4]}, total, threshold)
		require.NoError(t, err)
		require.Equal(t, secrets[v], back)
		polys = append(polys, [][]tbls.PublicKey{d.Commitments})
		good = append(good, v)
	}
	pubs, perrs, err := h.PublicKeyShares(polys, []int{1, 2, 3, 4})
	require.NoError(t, err)
	for k, v := range good {
		require.NoError(t, perrs[k])
		for idx, share := range dealt[v].Shares {
			pub, err := ref.SecretToPublicKey(share)
			require.NoError(t, err)
			require.Equal(t, pub, pubs[k][idx-1])
		}
	}

	none, errs, err := h.DealWithCommitments(nil, total, threshold)
	require.NoError(t, err)
	require.Nil(t, none)
	require.Nil(t, errs)
}

// TestVerifySecretSharesBatchEqualsHerumi: shares dealt by tbls.Herumi{}'s ThresholdSplit with threshold 1 (the share
// is the secret) pass against tbls.Herumi{}'s SecretToPublicKey of that secret as the only commitment, for every
// validator and dealer in one call; a flipped share, a foreign commitment list and a share above r are reported at
// exactly their (validator, dealer); the metrics advance under "verify_secret_shares".
func TestVerifySecretSharesBatchEqualsHerumi(t *testing.T) {
	h, err := New()
	require.NoError(t, err)
	ref := tbls.Herumi{}
	const nVal, dealers, myID = 3, 4, 2
	shares := make([][]tbls.PrivateKey, nVal)
	coms := make([][][]tbls.PublicKey, nVal)
	for v := range shares {
		for d := 0; d < dealers; d++ {
			secret, err := ref.GenerateSecretKey()
			require.NoError(t, err)
			dealt, err := ref.ThresholdSplit(secret, 4, 1)
			require.NoError(t, err)
			shares[v] = append(shares[v], dealt[myID])
			coms[v] = append(coms[v], commitments(t, []tbls.PrivateKey{secret}))
		}
	}

	items := func(path string) float64 { return promtest.ToFloat64(itemsCounter.WithLabelValues(path)) }
	failed := func(path string) float64 { return promtest.ToFloat64(failedCounter.WithLabelValues(path)) }
	i0, f0 := items("verify_secret_shares"), failed("verify_secret_shares")
	errs, err := h.VerifySecretSharesBatch(shares, coms, myID)
	require.NoError(t, err)
	require.InDelta(t, nVal*dealers, items("verify_secret_shares")-i0, 0)
	require.InDelta(t, 0, failed("verify_secret_shares")-f0, 0)
	for v := range errs {
		for d := range errs[v] {
			require.NoError(t, errs[v][d])
		}
	}

	// a forged share, two dealers' commitment lists exchanged, a share above r
	shares[0][1][31] ^= 1
	coms[1][3], coms[1][0] = coms[1][0], coms[1][3]
	for i := range shares[2][2] {
		shares[2][2][i] = 0xff // above r
	}
	errs, err = h.VerifySecretSharesBatch(shares, coms, myID)
	require.NoError(t, err)
	for v := range errs {
		for d := range errs[v] {
			switch {
			case v == 0 && d == 1, v == 1 && (d == 0 || d == 3):
				require.ErrorContains(t, errs[v][d], "secret share does not match the dealer's commitments")
			case v == 2 && d == 2:
				require.ErrorContains(t, errs[v][d], "cannot unmarshal bytes into Herumi secret key")
			default:
				require.NoError(t, errs[v][d])
			}
		}
	}

	// shares and commitments dealt on the device pass at every operator index
	secret, err := ref.GenerateSecretKey()
	require.NoError(t, err)
	dealt, derrs, err := h.DealWithCommitments([]tbls.PrivateKey{secret}, 4, 3)
	require.NoError(t, err)
	require.NoError(t, derrs[0])
	for idx, share := range dealt[0].Shares {
		errs, err = h.VerifySecretSharesBatch([][]tbls.PrivateKey{{share}}, [][][]tbls.PublicKey{{dealt[0].Commitments}}, idx)
		require.NoError(t, err)
		require.NoError(t, errs[0][0])
	}

	_, err = h.VerifySecretSharesBatch(shares, coms[:2], myID)
	require.Error(t, err)
}

// TestCombineSharesEqualsHerumi: three dealers deal with tbls.Herumi{}'s ThresholdSplit (2-of-3); every operator's sum
// of the shares it received is the host's sum mod r, its pubshare is tbls.Herumi{}'s SecretToPublicKey of that sum, and
// any two sums recover the sum of the dealers' secrets under tbls.Herumi{}'s RecoverSecret; an excluded dealer is left
// out of all of it; no included dealer is an error; the metrics advance under "combine_shares".
func TestCombineSharesEqualsHerumi(t *testing.T) {
	h, err := New()
	require.NoError(t, err)
	ref := tbls.Herumi{}
	const dealers, total, threshold = 3, 3, 2
	secrets := make([]tbls.PrivateKey, dealers)
	dealt := make([]map[int]tbls.PrivateKey, dealers)
	for d := range secrets {
		secrets[d], err = ref.GenerateSecretKey()
		require.NoError(t, err)
		dealt[d], err = ref.ThresholdSplit(secrets[d], total, threshold)
		require.NoError(t, err)
	}
	// one "validator" per operator index and mask: rows 0..2 take every dealer, rows 3..5 leave dealer 1 out, row 6 nobody
	var shares [][]tbls.PrivateKey
	var include [][]bool
	for _, mask := range [][]bool{{true, true, true}, {true, false, true}} {
		for idx := 1; idx <= total; idx++ {
			shares = append(shares, []tbls.PrivateKey{dealt[0][idx], dealt[1][idx], dealt[2][idx]})
			include = append(include, mask)
		}
	}
	shares = append(shares, shares[0])
	include = append(include, []bool{false, false, false})

	items := func(path string) float64 { return promtest.ToFloat64(itemsCounter.WithLabelValues(path)) }
	failed := func(path string) float64 { return promtest.ToFloat64(failedCounter.WithLabelValues(path)) }
	i0, f0 := items("combine_shares"), failed("combine_shares")
	sums, pubs, errs, err := h.CombineShares(shares, include)
	require.NoError(t, err)
	require.InDelta(t, len(shares), items("combine_shares")-i0, 0)
	require.InDelta(t, 1, failed("combine_shares")-f0, 0)
	require.Error(t, errs[6])
	for row := 0; row < 6; row++ {
		require.NoError(t, errs[row])
		want := sumModOrder(shares[row][0], shares[row][2])
		if include[row][1] {
			want = sumModOrder(shares[row][0], shares[row][1], shares[row][2])
		}
		require.Equal(t, want, sums[row])
		pub, err := ref.SecretToPublicKey(want)
		require.NoError(t, err)
		require.Equal(t, pub, pubs[row])
	}
	back, err := ref.RecoverSecret(map[int]tbls.PrivateKey{1: sums[0], 3: sums[2]}, total, threshold)
	require.NoError(t, err)
	require.Equal(t, sumModOrder(secrets...), back)
	back, err = ref.RecoverSecret(map[int]tbls.PrivateKey{2: sums[4], 3: sums[5]}, total, threshold)
	require.NoError(t, err)
	require.Equal(t, sumModOrder(secrets[0], secrets[2]), back)

	// a nil mask takes every dealer
	all, _, errs, err := h.CombineShares(shares[:3], nil)
	require.NoError(t, err)
	for row := range all {
		require.NoError(t, errs[row])
		require.Equal(t, sums[row], all[row])
	}
}
